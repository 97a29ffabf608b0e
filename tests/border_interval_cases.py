"""The per-border credible intervals (Aligner.set_border_interval; include/dynamont_mi.h) restated in
NumPy over the CPU oracle's lattices, the bounds the device is held to, and the read sets the tests share.

For output row j of a read: n = j + 1 is its lattice column and r = signal_positions[j] + 1 the row of its M cell. LPM(t, n) is
border_confidence_cases.lpm_columns' array: -inf outside the band window of row t and in row 0. p(t) = exp(LPM(t, n)) (0 where
LPM is -inf) for t = 1 .. T-1, a = (1 - mass) / 2; every sum is fp64, ascending t, one IEEE add per term (np.cumsum adds in
sequence, np.sum does not):
    C(t) = running sum of p,  S = C(T-1),  A = sum (t - r) * p,  B = sum ((t - r) * (t - r)) * p
    border_lo   = (first t with C(t) >= a) - 1
    border_hi   = (first t with C(t) >= 1 - a) - 1; a threshold no row reaches: the last in-band row of the column, minus 1
    border_mean = (r - 1) + A / S
    border_sd   = sqrt(max(B / S - (A / S)^2, 0))

The device reads a FLOAT log-posterior l (or rebuilds one of that accuracy): its p differs from exp(l) of the exact value by at
most 2^-24 p |ln p| relatively rounded, so per border
    tol_C = 1e-6 (border_confidence_cases.TOL: sum p |ln p| over a whole column stays below ln(rows))
    tol_A = 2^-23 * sum |d| p |ln p| + 1e-9,   tol_B = 2^-23 * sum d^2 p |ln p| + 1e-9          (d = t - r)
and a quantile cannot be held to one row where C passes the threshold within tol_C. The acceptance rule is total: a device row
t' is right for threshold q iff C(t') >= q - tol_C and C(t' - 1) < q + tol_C on the oracle's lattice (C(0) = 0) -- or, the
definition's fallback, t' is the column's last in-band row and the column's mass stays below q + tol_C.

`mutate` builds the deliberately wrong versions tests/test_border_interval_host.py holds the yardstick against."""
import numpy as np

import border_confidence_cases as bcc

TOL_C = bcc.TOL
MUTATIONS = ("greater_than", "one_sided_tail", "column_minus_one", "no_band_mask", "row_not_position")
MASSES = (0.5, 0.9, 0.999)


def last_band_rows(orc, T, N, band):
    """last in-band row of every column (0: the column is never in band)"""
    bw = min(band // 2, N // 2)
    _, n_start, n_end = orc.bounds(T, N, bw)
    last = np.zeros(N, dtype=np.int64)
    for t in range(1, T):
        last[max(int(n_start[t]), 1):int(n_end[t])] = t
    return last


class Column:
    """one border's column on the oracle's lattice: the running sum and what the bounds need"""

    def __init__(self, col, r):
        with np.errstate(invalid="ignore"):
            p = np.exp(col[1:])                                   # rows 1 .. T-1; exp(-inf) = 0
        t = np.arange(1, len(col))
        d = (t - r).astype(np.float64)
        self.C = np.concatenate(([0.0], np.cumsum(p)))            # C[t], C[0] = 0
        self.S = float(self.C[-1])
        self.A = float(np.cumsum(d * p)[-1])
        self.B = float(np.cumsum((d * d) * p)[-1])
        with np.errstate(invalid="ignore", divide="ignore"):
            plnp = np.where(p > 0, p * np.abs(np.log(np.where(p > 0, p, 1.0))), 0.0)
        self.tol_A = 2.0 ** -23 * float(np.sum(np.abs(d) * plnp)) + 1e-9
        self.tol_B = 2.0 ** -23 * float(np.sum(d * d * plnp)) + 1e-9

    def first(self, q, strict=False):
        """first row t with C(t) >= q (strict: > q), or 0"""
        hit = self.C[1:] > q if strict else self.C[1:] >= q
        return int(np.argmax(hit)) + 1 if hit.any() else 0

    def near(self, q):
        """whether the threshold lies within tol_C of some C(t)"""
        return bool((np.abs(self.C[1:] - q) <= TOL_C).any())


def accepts(colm, q, row, last):
    """the acceptance rule for a device quantile ROW (position + 1)"""
    if row < 1 or row >= len(colm.C):
        return False
    if colm.C[row] >= q - TOL_C and colm.C[row - 1] < q + TOL_C:
        return True
    return row == last and colm.S < q + TOL_C


def from_lpm(lpm, rows, last, mass, mutate=None):
    """(border_lo, border_hi, border_mean, border_sd, columns) along the borders `rows` over an LPM array [T, N]; `last` =
    last_band_rows; columns[j] is the Column of border j (of the column the mutation looks at, if any)"""
    a = 1.0 - mass if mutate == "one_sided_tail" else (1.0 - mass) / 2
    m = len(rows)
    lo, hi = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    mean, sd = np.zeros(m), np.zeros(m)
    cols = []
    for j, r in enumerate(int(x) for x in rows):
        n = j + 1
        if mutate == "column_minus_one":
            n = max(n - 1, 1)
        c = Column(lpm[:, n], r)
        cols.append(c)
        back = 0 if mutate == "row_not_position" else 1
        t_lo = c.first(a, mutate == "greater_than") or int(last[n])
        t_hi = c.first(1.0 - a, mutate == "greater_than") or int(last[n])
        lo[j], hi[j] = t_lo - back, t_hi - back
        mean[j] = (r - back) + c.A / c.S
        sd[j] = np.sqrt(max(c.B / c.S - (c.A / c.S) ** 2, 0.0))
    return lo, hi, mean, sd, cols


class Yard:
    """the yardstick of one read at one band: the lattice is computed once, every mass asks it again"""

    def __init__(self, orc, signal, seq, band=400):
        self.orc, self.signal, self.seq, self.band = orc, signal, seq, band
        self.lpm, self.res = bcc.lpm_columns(orc, signal, seq, band)
        self.T, self.N = self.lpm.shape
        self.rows = self.res["signal_positions"].astype(np.int64) + 1
        self.last = last_band_rows(orc, self.T, self.N, band)
        self._cache = {}

    def at(self, mass, mutate=None):
        key = (mass, mutate)
        if key not in self._cache:
            lpm = self.lpm
            if mutate == "no_band_mask":
                lpm, _ = bcc.lpm_columns(self.orc, self.signal, self.seq, self.band, res=self.res, mask=False)
            self._cache[key] = from_lpm(lpm, self.rows, self.last, mass, mutate)
        return self._cache[key]

    def window_mass(self, W):
        return bcc.from_lpm(self.lpm, self.rows, W)[1]


def check_device(y, mass, lo, hi, mean, sd, what):
    """hold one read's four device columns to the yardstick; returns (borders whose quantile differs from the oracle's own,
    largest mean error / its bound, largest variance error / its bound). No border is left out of any comparison."""
    ylo, yhi, ymean, ysd, cols = y.at(mass)
    a = (1.0 - mass) / 2
    m = len(cols)
    assert len(lo) == len(hi) == len(mean) == len(sd) == m, (what, m, len(lo))
    moved, worst_m, worst_v = 0, 0.0, 0.0
    for j, c in enumerate(cols):
        n = j + 1
        for q, got, name in ((a, int(lo[j]), "lo"), (1.0 - a, int(hi[j]), "hi")):
            assert accepts(c, q, got + 1, int(y.last[n])), (what, name, j, got, int((ylo, yhi)[name == "hi"][j]), c.C[max(got, 0):got + 3].tolist(), q)
        moved += int(lo[j] != ylo[j]) + int(hi[j] != yhi[j])
        bound_m = c.tol_A / c.S
        err_m = abs(float(mean[j]) - float(ymean[j]))
        assert err_m <= bound_m, (what, "mean", j, float(mean[j]), float(ymean[j]), bound_m)
        # var = B / S - m^2 with m = A / S: |d var| <= tol_B / S + 2 |m| tol_A / S + (tol_A / S)^2
        mo = abs(c.A / c.S)
        bound_v = c.tol_B / c.S + 2.0 * mo * bound_m + bound_m ** 2
        err_v = abs(float(sd[j]) ** 2 - float(ysd[j]) ** 2)
        assert err_v <= bound_v, (what, "variance", j, float(sd[j]) ** 2, float(ysd[j]) ** 2, bound_v)
        worst_m, worst_v = max(worst_m, err_m / bound_m), max(worst_v, err_v / bound_v)
    print(f"{what} mass={mass}: {m} borders, {moved} quantiles off the oracle's own row (all accepted), "
          f"mean error <= {worst_m:.3f} of its bound, variance error <= {worst_v:.3f} of its bound")
    return moved, worst_m, worst_v


def conditions(yards, mass=0.9):
    """the read sets' conditions: (share of borders with hi > lo, widest interval in rows, share of borders with a threshold within
    tol_C of some C(t))"""
    wide = total = near = 0
    widest = 0
    a = (1.0 - mass) / 2
    for y in yards:
        lo, hi, _, _, cols = y.at(mass)
        total += len(cols)
        wide += int((hi > lo).sum())
        widest = max(widest, int((hi.astype(np.int64) - lo.astype(np.int64)).max()))
        near += sum(c.near(a) or c.near(1.0 - a) for c in cols)
    return wide / total, widest, near / total


def assert_conditions(yards, what, mass=0.9):
    share, widest, near = conditions(yards, mass)
    print(f"{what}: {100 * share:.1f} % of the borders have hi > lo, widest interval {widest} rows, "
          f"{100 * near:.2f} % of the borders have a threshold within tol_C of a C(t)")
    assert share >= 0.20 and widest >= 16 and near <= 0.01, (what, share, widest, near)


# ---- the read sets (dynamont_amd.synth, fixed seeds) --------------------------------------------------------------------------------
PLAIN_SEED, LONG_SEED, IMPERFECT_SEED = 11, 12, 13


def read_sets(models):
    """name -> (model key, pore, band, reads)"""
    plain = bcc.plain_reads(models["syn9"], "rna004", PLAIN_SEED, 6, 150)
    long_ = bcc.plain_reads(models["syn9"], "rna004", LONG_SEED, 3, 700)       # more than 448 columns: the band slots wrap
    imperfect = bcc.imperfect_reads(models["syn5"], "rna002", IMPERFECT_SEED, 4, 300)
    return {
        "plain": ("syn9", "rna004", 400, plain),
        "plain_band50": ("syn9", "rna004", 50, plain),
        "long": ("syn9", "rna004", 400, long_),
        "long_band50": ("syn9", "rna004", 50, long_),
        "imperfect": ("syn5", "rna002", 400, imperfect),
        # the same reads at band 50: the path runs along the band's edge, where an unmasked read of a band slot carries mass
        "imperfect_band50": ("syn5", "rna002", 50, imperfect),
    }


def tie_lattice():
    """(LPM [T, N], rows, last) of a lattice whose running sums MEET the thresholds of mass 0.5 exactly: every column holds four
    rows of mass exactly 0.25 (C = 0.25, 0.5, 0.75, 1), so `>=` answers rows 1 and 3 of the four and `>` rows 2 and 4. On
    the read sets no C(t) equals a threshold (0 of about 12 000), and the two cannot be told apart there."""
    import math
    T, N = 40, 9
    quarter = math.log(0.25)
    assert math.exp(quarter) == 0.25
    lpm = np.full((T, N), -np.inf)
    rows, last = np.zeros(N - 1, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for n in range(1, N):
        lpm[4 * n:4 * n + 4, n] = quarter
        rows[n - 1], last[n] = 4 * n + 1, 4 * n + 3
    return lpm, rows, last


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
