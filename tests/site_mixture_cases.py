"""The per-site two-component mixture fit (dyn_aligner_site_mixture) restated in Python floats: one IEEE
fp64 operation per operation of the definition and the definition's one summation tree (gsum). exp is the library's strict exp
built for the host with g++ from dp_math_strict.hpp (tests/device_math/site_mixture_host.cpp), not math.exp: the restatement does
not depend on the host's libm. Also the case tables and the windows of the device harness (tests/device_math/site_mixture.hip).

``fit(..., wrong=...)`` restates WRONG versions a kernel could compute instead; tests/test_site_mixture_host.py asserts that the
built sites tell each of them from the definition."""
import atexit
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = (1 << 32) - 1
DWELL_BINS = 16
NAN = float("nan")
DOUBLES = ("pi1", "mu0", "mu1", "var0", "var1", "r_a", "r_b")
COUNTS = ("n_a", "n_b", "out_a", "out_b", "iters", "status")
COLUMNS = DOUBLES + COUNTS
DEFAULTS = dict(max_iters=128, tol=1e-3, min_n=8)
WRONG = ("keeps_updating", "outliers_in_fit", "count_wraps", "stale_g", "labels_not_in_shares")

_LIB = None


def exp_lib():
    """tests/device_math/site_mixture_host.cpp built with g++ -O2 -ffp-contract=off (as tests/test_dp_math_strict.py builds its
    library), once per process"""
    global _LIB
    if _LIB is None:
        d = tempfile.mkdtemp(prefix="dyn_smix_")
        atexit.register(shutil.rmtree, d, True)
        so = os.path.join(d, "libsmix_host.so")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "dynamont_amd", "csrc"), "-o", so,
                        os.path.join(ROOT, "tests", "device_math", "site_mixture_host.cpp")], check=True)
        _LIB = C.CDLL(so)
        _LIB.exp_strict.restype = C.c_double
        _LIB.exp_strict.argtypes = [C.c_double]
        _LIB.exp_strict_n.restype = None
    return _LIB


def exp_strict(x):
    return exp_lib().exp_strict(float(x))


def exp_many(args):
    n = len(args)
    src = (C.c_double * n)(*args)
    dst = (C.c_double * n)()
    exp_lib().exp_strict_n(src, dst, C.c_long(n))
    return list(dst)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def group_width(bc):
    g = 4
    while g < bc and g < 64:
        g <<= 1
    return g


def gsum(terms, g):
    """lane l owns e = r * G + l: a partial from +0.0 in rising r (an index >= Bc adds 0.0), then the xor tree over the G partials"""
    n = len(terms)
    part = []
    for lane in range(g):
        s = 0.0
        for e in range(lane, max(n, lane + 1), g):
            s = s + (terms[e] if e < n else 0.0)
        part.append(s)
    m = 1
    while m < g:
        part = [part[lane] + part[lane ^ m] for lane in range(g)]
        m <<= 1
    return part[0]


def constants(bins, lo, hi, tol):
    w = (hi - lo) / bins
    return w, (w * w) / 12.0, tol * w, tol


def centres(bins, lo, hi):
    w = (hi - lo) / bins
    return [lo + (float(e) - 0.5) * w for e in range(bins + 2)]


def estep(x, mu, var, pi):
    amp = [pi[k] / math.sqrt(var[k]) for k in (0, 1)]
    q0, q1, args = [], [], []
    for xe in x:
        d0, d1 = xe - mu[0], xe - mu[1]
        a0, a1 = -0.5 * ((d0 * d0) / var[0]), -0.5 * ((d1 * d1) / var[1])
        qm = a1 if a1 > a0 else a0
        args.append(a0 - qm)
        args.append(a1 - qm)
    ex = exp_many(args)
    g0, g1 = [], []
    for e in range(len(x)):
        p0, p1 = amp[0] * ex[2 * e], amp[1] * ex[2 * e + 1]
        s = p0 + p1
        g0.append(p0 / s)
        g1.append(p1 / s)
    return g0, g1


def fit(a, b, bins, lo, hi, max_iters=128, tol=1e-3, min_n=8, trace=None, wrong=None):
    """one pair: a, b lists of bins + 2 ints (b None: the single-sample form). Returns the thirteen outputs. ``trace`` (a list)
    receives (mu, var, pi) at the start and after every adopted round. ``wrong``: one of WRONG."""
    bc = bins + 2
    a = [int(v) for v in a]
    b = [0] * bc if b is None else [int(v) for v in b]
    assert len(a) == bc and len(b) == bc
    g = group_width(bc)
    w, vfloor, tol_mu, tol_pi = constants(bins, lo, hi, tol)
    x = centres(bins, lo, hi)
    fit_range = range(bc) if wrong == "outliers_in_fit" else range(1, bc - 1)
    c = [0.0] * bc
    for e in fit_range:
        c[e] = float((a[e] + b[e]) & M32) if wrong == "count_wraps" else float(a[e]) + float(b[e])   # (a uint32 sum)
    out = dict(n_a=sum(a[1:-1]) & M32, n_b=sum(b[1:-1]) & M32, out_a=(a[0] + a[-1]) & M32, out_b=(b[0] + b[-1]) & M32, iters=0, status=1)
    out.update({k: NAN for k in DOUBLES})
    n = gsum(c, g)
    if n < min_n:
        return out
    m = gsum([c[e] * x[e] for e in range(bc)], g) / n
    v = gsum([c[e] * ((x[e] - m) * (x[e] - m)) for e in range(bc)], g) / n
    if not v > vfloor:
        return out
    sd = math.sqrt(v)
    mu, var, pi = [m - sd, m + sd], [v, v], [0.5, 0.5]
    if trace is not None:
        trace.append((list(mu), list(var), list(pi)))
    status, iters, done = 2, 0, False
    last_g = None
    for it in range(1, max_iters + 1):
        gk = estep(x, mu, var, pi)
        t = [[c[e] * gk[k][e] for e in range(bc)] for k in (0, 1)]
        big = [gsum(t[k], g) for k in (0, 1)]
        if big[0] < 1.0 or big[1] < 1.0:
            if not done:
                status = 3
            break
        nm = [gsum([t[k][e] * x[e] for e in range(bc)], g) / big[k] for k in (0, 1)]
        nv = []
        for k in (0, 1):
            q = gsum([t[k][e] * ((x[e] - nm[k]) * (x[e] - nm[k])) for e in range(bc)], g) / big[k]
            nv.append(vfloor if vfloor > q else q)
        tot = big[0] + big[1]
        npi = [big[0] / tot, big[1] / tot]
        d0, d1 = abs(nm[0] - mu[0]), abs(nm[1] - mu[1])
        dm = d1 if d1 > d0 else d0
        dp = abs(npi[1] - pi[1])
        mu, var, pi = nm, nv, npi
        last_g = gk
        if not done:
            iters = it
            if trace is not None:
                trace.append((list(mu), list(var), list(pi)))
            if dm <= tol_mu and dp <= tol_pi:
                status = 0
                if wrong != "keeps_updating":
                    break
                done = True     # the wrong version: status and iters stand, the parameters go on moving
    gk = last_g if wrong == "stale_g" and last_g is not None else estep(x, mu, var, pi)
    swap = mu[0] > mu[1]
    gs = gk[0] if swap and wrong != "labels_not_in_shares" else gk[1]
    inner = lambda e: 0 < e < bc - 1  # noqa: E731
    r_a = gsum([float(a[e]) * gs[e] if inner(e) else 0.0 for e in range(bc)], g)
    r_b = gsum([float(b[e]) * gs[e] if inner(e) else 0.0 for e in range(bc)], g)
    k0, k1 = (1, 0) if swap else (0, 1)
    out.update(pi1=pi[k1], mu0=mu[k0], mu1=mu[k1], var0=var[k0], var1=var[k1], r_a=r_a, r_b=r_b, iters=iters, status=status)
    return out


_CACHE = {}


def fit_arrays(level, site_lo, other_lo, count, spec, key=None, **params):
    """the thirteen columns over the pairs (site_lo + i, other_lo + i) of level [n][Bc] (lists of lists of ints); other_lo None: the
    single-sample form. ``key``: a hashable name of the table, to share a pair's fit among the windows and tests that meet it."""
    rows = []
    for i in range(count):
        k = None if key is None else (key, site_lo + i, None if other_lo is None else other_lo + i, tuple(sorted(params.items())))
        if k is None or k not in _CACHE:
            r = fit(level[site_lo + i], None if other_lo is None else level[other_lo + i], *spec, **params)
            if k is None:
                rows.append(r)
                continue
            _CACHE[k] = r
        rows.append(_CACHE[k])
    return {c: np.array([r[c] for r in rows], dtype=np.float64 if c in DOUBLES else np.uint32) for c in COLUMNS}


def same_bits(got, want):
    """None, or the first column and pairs at which two dicts of columns differ (doubles by their bit patterns)"""
    for c in COLUMNS:
        g, w = np.ascontiguousarray(got[c]), np.ascontiguousarray(want[c])
        if g.dtype != w.dtype or g.shape != w.shape:
            return c, "dtype / shape", str((g.dtype, g.shape, w.dtype, w.shape))
        gb, wb = (g.view(np.uint64), w.view(np.uint64)) if c in DOUBLES else (g, w)
        bad = np.flatnonzero(gb != wb)
        if bad.size:
            return c, bad[:6].tolist(), "got %s want %s" % (g[bad[:6]].tolist(), w[bad[:6]].tolist())
    return None


def log_likelihood(a, b, bins, lo, hi, mu, var, pi):
    """of the binned data (the pooled in-range counts as point masses at the bin centres), with math.log: for the tests only"""
    x = centres(bins, lo, hi)
    ll = 0.0
    for e in range(1, bins + 1):
        ce = int(a[e]) + (0 if b is None else int(b[e]))
        if ce:
            dens = sum(pi[k] / math.sqrt(2.0 * math.pi * var[k]) * math.exp(-0.5 * (x[e] - mu[k]) ** 2 / var[k]) for k in (0, 1))
            ll += ce * math.log(dens)
    return ll


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def two_condition(rng, bins, lo, hi, n_a, n_b, share, shift, sd):
    """A: n_a values around one level; B: n_b values of which ``share`` sit ``shift`` higher. Returns the two counter rows."""
    span = hi - lo
    centre = lo + span * rng.uniform(0.3, 0.5)
    k = int(round(share * n_b))
    va = rng.normal(centre, sd * span, n_a)
    vb = np.concatenate([rng.normal(centre, sd * span, n_b - k), rng.normal(centre + shift * span, sd * span, k)])
    return histogram(va, bins, lo, hi), histogram(vb, bins, lo, hi)


def histogram(values, bins, lo, hi):
    h = [0] * (bins + 2)
    for v in np.asarray(values, dtype=np.float64).tolist():
        u = (v - lo) * (bins / (hi - lo))
        h[0 if u < 0 else (bins + 1 if u >= bins else 1 + int(u))] += 1
    return h


def random_row(rng, bins, lo, hi, style):
    """seeded single rows of every temper: sparse Poisson counts (slow or no convergence), a narrow cluster plus a stray (collapses),
    samples of one Gaussian, of two; style 4: a cluster in one bin and one stray row two to four bins above it"""
    row = [0] * (bins + 2)
    if style == 0:
        row[1:-1] = [int(v) for v in rng.poisson(rng.uniform(0.05, 3), bins)]
    elif style == 1:
        c = int(rng.integers(2, bins))
        for e in (c - 1, c, c + 1):
            if 1 <= e <= bins:
                row[e] = int(rng.integers(0, 400))
        row[int(rng.integers(1, bins + 1))] += int(rng.integers(0, 3))
    elif style == 4:
        c = int(rng.integers(1, bins - 4))
        row[c], row[c + int(rng.integers(2, 5))] = int(rng.integers(10, 60)), 1
    elif style == 2:
        span = hi - lo
        row = histogram(rng.normal(lo + span * rng.uniform(0.25, 0.75), span * rng.uniform(0.02, 0.12), int(rng.integers(8, 200))), bins, lo, hi)
    else:
        row = [p + q for p, q in zip(*two_condition(rng, bins, lo, hi, int(rng.integers(30, 300)), int(rng.integers(30, 300)),
                                                    rng.uniform(0.1, 0.9), rng.uniform(0.15, 0.4), rng.uniform(0.02, 0.06)))]
    if rng.random() < 0.3:
        row[0] += int(rng.integers(0, 50))
        row[-1] += int(rng.integers(0, 50))
    return row


# the host test's table: 32 bins, the defaults
HOST_SPEC = (32, -4.0, 4.0)


def host_cases(n=200, seed=4100):
    """about 200 seeded two-condition histograms (a, b) at HOST_SPEC, 60 to 4 000 reads"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        n_a, n_b = (int(v) for v in rng.integers(30, 2000, 2))
        out.append(two_condition(rng, *HOST_SPEC, n_a, n_b, rng.uniform(0.0, 0.9), rng.uniform(0.05, 0.3), rng.uniform(0.03, 0.07)))
    return out


def status_cases(n=150, seed=4200):
    """seeded single rows of all five tempers at HOST_SPEC: every status code occurs among them"""
    rng = np.random.default_rng(seed)
    return [random_row(rng, *HOST_SPEC, i % 5) for i in range(n)]


# ---- the harness inputs --------------------------------------------------------------------------------------------------------------
N_SITES, PAIRS = 80, 37
WIDTHS = (8, 18, 34, 66, 130, 256)
H_LO, H_HI = -3.7, 4.1                                  # a bin width that is no power of two
H_PARAMS = dict(max_iters=24, tol=1e-3, min_n=8)
# (site_lo, other_lo, count): the built pairs with the other window BELOW; a window overlapping itself by half; one pair starting at the
# table's last site; a window against itself; the single-sample form (other_lo None)
WINDOWS = ((40, 0, PAIRS), (3, 21, PAIRS), (N_SITES - 1, 5, 1), (7, 7, PAIRS), (40, None, PAIRS))
BUILT = ("fast", "slow", "fast_again", "empty_a", "empty_b", "empty_both", "one_bin", "below_min_n", "at_min_n", "collapse", "top",
         "outside_only", "outliers", "crossing")


def spec_of(w):
    return (w - 2, H_LO, H_HI)


def pattern(kind, w, rng):
    """two level-counter rows of width w = bins + 2"""
    bins = w - 2
    a, b = [0] * w, [0] * w
    p, q = 1 + bins // 5, bins - bins // 6               # two in-range bins far apart
    if kind in ("fast", "fast_again"):                   # all of A in one bin, all of B in another: a handful of rounds
        a[p], b[q] = 300, 700
    elif kind == "slow":                                 # sparse counts all over the range: EM creeps, max_iters ends it
        if bins < 32:
            for e in range(1, bins + 1):
                a[e] = 1 + (e * 7) % 3
                b[e] = 1 + (e * 5) % 4
        else:
            a[1:-1] = [int(v) for v in np.random.default_rng(500 + w).poisson(1.0, bins)]
            b[1:-1] = [int(v) for v in np.random.default_rng(900 + w).poisson(0.6, bins)]
            a[1] += 2
            b[bins] += 2
    elif kind == "empty_a":
        b[p], b[q] = 40, 25
    elif kind == "empty_b":
        a[p], a[q] = 25, 40
    elif kind == "one_bin":                              # no spread: v = 0 is not above the floor
        a[p], b[p] = 30, 12
    elif kind == "below_min_n":
        a[p], b[q] = 4, H_PARAMS["min_n"] - 5
    elif kind == "at_min_n":
        a[p], b[q] = 4, H_PARAMS["min_n"] - 4
    elif kind == "collapse":                             # a cluster and one stray row next to it: the second component starves
        a[p], a[p + 2] = 20, 1
    elif kind == "top":                                  # 2^32 - 1 rows on both sides in different bins: the pooled count needs 33 bits
        a[p], b[q] = M32 - 3, M32
        a[q] = 3                                         # ... and so does bin q's own
    elif kind == "outside_only":
        a[0], a[w - 1], b[0] = 9, 5, 7
    elif kind == "outliers":                             # "fast" with large under / over counters on both sides
        a[p], b[q] = 300, 700
        a[0], a[w - 1], b[0], b[w - 1] = 5000, M32, 123456, 77
    elif kind == "crossing":                             # see crossing_row
        a = crossing_row(bins)
    elif kind != "empty_both":
        raise ValueError(kind)
    return a, b


def crossing_row(bins):
    """a row whose final means cross (mu_0 > mu_1 before the labels are exchanged): a cluster of two neighbouring bins, the heavier
    one below, and a stray row six bins under it (six bins and few: a slope under a heavy cluster). Found with the restatement;
    tests/test_site_mixture_host.py asserts that the exchange runs."""
    row = [0] * (bins + 2)
    if bins >= 12:
        p = (3 * bins) // 4
        row[p], row[p + 1], row[p - 6] = 129, 32, 1
        return row
    hi_bin = bins - max(1, bins // 8)
    row[hi_bin] = 900
    if hi_bin + 1 <= bins:
        row[hi_bin + 1] = 40
    for e in range(1, hi_bin):
        row[e] = 1 + (e % 2)
    return row


def mixture_tables():
    """{Bc: uint32 [N_SITES][Bc + 16]}: pair i of WINDOWS[0] (A = 40 + i, B = i) holds BUILT[i] in its level counters; everything else
    seeded random rows of every temper; the dwell counters random (the fit does not read them)"""
    out = {}
    for w in WIDTHS:
        rng = np.random.default_rng(8800 + w)
        bins = w - 2
        t = np.zeros((N_SITES, w + DWELL_BINS), dtype=np.uint32)
        for s in range(N_SITES):
            t[s, :w] = random_row(rng, bins, H_LO, H_HI, s % 4)
            t[s, w:] = rng.integers(0, 1 << 20, DWELL_BINS)
        for i, kind in enumerate(BUILT):
            a, b = pattern(kind, w, rng)
            t[40 + i, :w] = a
            t[i, :w] = b
        out[w] = t
    return out


def level_of(table, w):
    return table[:, :w].tolist()
