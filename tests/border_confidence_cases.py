"""The per-border posterior confidence (Aligner.set_border_confidence; include/dynamont_mi.h)
restated in NumPy over the CPU oracle's lattices, and the read sets the tests share.

For output row j of a read: n = j + 1 is its lattice column and r = signal_positions[j] + 1 the row of its M cell. With
LPM(t, n) = fM(t, n) + bM(t, n) - Z, taken as -inf for every cell outside the band window of row t and in row 0,
    border_probability[j]         = exp(LPM(r, n))
    border_window_probability[j]  = sum over t = max(1, r - W) .. min(T - 1, r + W) of exp(LPM(t, n)), ascending t, not clamped
The lattices are Oracle.debug_fb's (band column c of row t <-> lattice column start[t] + c, as tests/path_posteriors.py
addresses them), the band window Oracle.bounds'.

`mutate` builds the deliberately wrong versions tests/test_border_confidence_host.py holds the yardstick against."""
import math

import numpy as np

import path_posteriors  # noqa: F401  (the band-column addressing used below is the one it documents)
from dynamont_amd import synth

TOL = 1e-6  # 2^-24 p |ln p| per term (the float log-posterior), sum p |ln p| <= ln(2 W + 1): at most 3.7e-7 at W = 256
MUTATIONS = ("window_minus_one", "window_shifted", "column_minus_one", "no_band_mask")


def lpm_columns(orc, signal, seq, band=400, res=None, mask=True):
    """(LPM [T, N] with -inf outside the band window and in row 0, res). mask=False: an out-of-band cell takes the value of the
    nearest in-band cell of its row instead (what an unmasked read of a band slot may return) -- a mutation."""
    res = res or orc.align(signal, seq, True)
    T, N = len(signal) + 1, len(seq) - orc.k + 2
    bw = min(band // 2, N // 2)
    fb = orc.debug_fb(signal, seq, 2 * bw + 1)
    start, n_start, n_end = orc.bounds(T, N, bw)
    lpm = np.full((T, N), -np.inf)
    for t in range(1, T):
        lo, hi = max(int(n_start[t]), 1), int(n_end[t])          # the forward sweep never fills column 0
        n = np.arange(lo, hi)
        c = n - int(start[t])
        assert (c >= 0).all() and (c < 2 * bw + 1).all()
        lpm[t, lo:hi] = fb["fM"][t, c] + fb["bM"][t, c] - res["Z"]
        if not mask:
            lpm[t, :lo] = lpm[t, lo]
            lpm[t, hi:] = lpm[t, hi - 1]
    return lpm, res


def from_lpm(lpm, rows, W, mutate=None):
    """the two columns along the borders `rows` (row of every segment's M cell) over an LPM array [T, N]"""
    T = lpm.shape[0]
    bp, bwp = np.zeros(len(rows)), np.zeros(len(rows))
    for j, r in enumerate(int(x) for x in rows):
        n = j + 1
        w, centre = W, r
        if mutate == "window_minus_one":
            w = W - 1
        elif mutate == "window_shifted":
            centre = r + 1
        elif mutate == "column_minus_one":
            n = max(n - 1, 0)
        bp[j] = math.exp(lpm[r, n])
        s = 0.0
        for t in range(max(1, centre - w), min(T - 1, centre + w) + 1):
            s += math.exp(lpm[t, n])                                  # ascending t, one IEEE add per term
        bwp[j] = s
    return bp, bwp


def yardstick(orc, signal, seq, W, band=400, res=None, mutate=None):
    """(border_probability, border_window_probability, res) of one read"""
    lpm, res = lpm_columns(orc, signal, seq, band, res, mask=mutate != "no_band_mask")
    rows = res["signal_positions"].astype(np.int64) + 1
    bp, bwp = from_lpm(lpm, rows, W, mutate)
    return bp, bwp, res


def window_counts(T, N, band, rows, W):
    """(windows cut at row 1 or T - 1, windows that hold at least one out-of-band row) of a read's borders"""
    bw = min(band // 2, N // 2)
    ratio = N / T
    clipped = leaving = 0
    for j, r in enumerate(int(x) for x in rows):
        n = j + 1
        clipped += (r - W < 1) or (r + W > T - 1)
        out = False
        for t in range(max(1, r - W), min(T - 1, r + W) + 1):
            mid = int(t * ratio)
            if not (max(mid - bw, 1) <= n < min(mid + bw + 1, N)):
                out = True
                break
        leaving += out
    return clipped, leaving


# ---- the read sets (dynamont_amd.synth, fixed seeds; their stated properties are asserted on the CPU oracle in
# tests/test_border_confidence_host.py and again, on the yardstick, where the GPU tests use them) ----------------------------
def model_tables(model):
    _, mean, sd = synth.read_model_file(model)
    return mean, sd


def plain_reads(model, pore, seed, n, n_bases):
    mean, sd = model_tables(model)
    return synth.make_reads(seed, n, pore, mean, sd, n_bases)


def imperfect_reads(model, pore, seed, n, n_bases):
    """5 % substitutions, 3 % indels, heavy-tailed dwell (synth.imperfect_read): the path strays from the band's diagonal"""
    mean, sd = model_tables(model)
    _, rna, k = synth.PORES[pore]
    mean_c, sd_c = synth.code_order_table(mean, sd, k, rna)
    rng = np.random.default_rng(seed)
    return [synth.imperfect_read(rng, mean_c, sd_c, k, n_bases, True, 0.05, 0.03, rna) for _ in range(n)]


RNA002_SEED, DNA_R9_SEED = 1, 11        # test 1: 3 reads each, 120 / 200 bases
CLIPPED_SEED = 5                        # test 2: 3 rna002 reads of 60 bases, W = 64
BAND50_SEED, BAND50_LONG_SEED = 3, 3    # test 3: dna_r9 imperfect reads at band = 50, 200 and 600 bases
WIDE_SEED = 21                          # test 5: one rna002 read of 600 bases at band = 600
