"""Shared by tests/test_any_band_host.py, tests/test_gpu_any_band.py and tests/test_gpu_parity.py (no GPU, no library): the read
sets that put the diagonal any-band kernel (k_band_reads<DiagonalWindow, 256, 16, ..> of band_reads.hip, with and without
lattice phases) on REUSED workgroups with reads of MIXED width, and the bar a wide-band train() result is held to against
``Oracle.train(.., dense=False)``.

Read sets (``read_sets``). Model syn5, pore dna_r9 (k = 5, no polyA pad: N = k-mer count + 1 = bases - 3, as launch.cpp forms it),
handle band 1 000, so bw = min(500, N / 2) and B = 2 bw + 3 is the read's own:
  W   14 wide reads (bw > 223). B = 451 (the narrowest wide read), 511 (thread 255 has no k = 1 column), 513 (thread 0 alone has
      a k = 2 column), 767, 769 and 1 003 (N >= 1 000), at dwell 2.0 (T a little above 2 N: the band moves about every second
      row and a running sum of the train job covers 1-2 rows before it is flushed) and, for the narrow ones, at dwell 10 (a
      running sum covers ~10 rows); one read with a homopolymer of 2 k bases (a structural tie), one with a NaN sample at its
      middle (the reference lets NaN through its Z check; this build fails the read).
  S   6 short reads (N < 448), which the register sweeps take in the same batch.
``orders(W)``: W sorted by B descending (a narrow read follows a wide one on a workgroup: stale LDS and arena beyond the new B)
and ascending (the converse). Two workgroups (DYN_QUEUE_CUS=2) take the 14 reads off the queue in that order.

The train bar (``train_bar``), derived, not measured. For a k-mer code that labels c lattice columns of a read with T rows the
weight is a sum of at most m = c (T - 1) terms g = exp((fM + bM) - Zb) + exp((fE + bE) - Zb), all >= 0. The kernel's operands of
exp are the reference's bit for bit (dp_math_strict.hpp restates the reference's log-domain arithmetic operation by operation),
so with u = 2^-53 a term differs between the two by
  the two exp implementations (the oracle's libm, the device's): each documented at <= 1 ulp = 2 u relative, on two exps whose
  sum is their weighted mean                                                                                     <= 4 u
  the rounding of the sum of the two exp values, once per side                                                   <= 2 u
and the sums differ by the order in which m non-negative terms are added (the oracle: rows outside, columns inside, straight
into the k-mer's word; the kernel: per thread over the rows between two band shifts, flushed into the column's word, columns
grouped by code on the host): recursive summation of m non-negative terms in ANY order and grouping is within (m - 1) u of the
exact sum to first order, on either side                                                                         <= 2 (m - 1) u
-- together (2 m + 4) u; the products g x and (g x) x are formed alike on both sides (one rounding each, of a term that already
differs by 6 u). The bar is
  weight, sumsq   |d| <= (2 m + 12) u |ref|            (8 u of room for the second-order terms: m u < 1e-9 here)
  sum             |d| <= (2 m + 12) u weight_ref max|x|   (signed terms can cancel: the weight's bar carried through the sum)
with no absolute term: every column's exact weight is >= 1, because a path spends at least one row in each column. The other
checks keep the project's bars: touched codes (weight > 0) equal as sets, Z equal in bits, m1 / e2 within 1e-8, sum(weight)
within 1e-8 S of S. Two conditions hold for every k-mer of every read of W (tests/test_any_band_host.py): the bar is <= 1e-9,
a hundred times inside the rtol = 1e-7 it stands beside, and never below 16 u.
What the device reaches is in profiles/any_band/train_bar.txt."""
from types import SimpleNamespace

import numpy as np

from dynamont_amd import synth

MODEL, PORE, BAND, K = "syn5", "dna_r9", 1000, 5
U = 2.0 ** -53
WIDE_ABOVE = 223   # half bands the register sweeps hold (band_reads.hip)

# (name, lattice columns N, dwell, kind); bases = N + K - 2
WIDE = (("b451_d2", 448, 2.0, ""), ("b451_d10", 449, 10.0, ""),
        ("b511_d2", 508, 2.0, ""), ("b511_d10", 509, 10.0, ""),
        ("b513_d2", 510, 2.0, ""), ("b513_d10", 511, 10.0, ""),
        ("b767_d2", 764, 2.0, ""), ("b767_tie", 765, 2.0, "tie"),
        ("b769_d2", 766, 2.0, ""), ("b769_odd", 767, 2.0, ""),
        ("b1003_d2", 1000, 2.0, ""), ("b1003_long", 1040, 2.0, ""),
        ("b513_nan", 511, 2.0, "nan"), ("b511_odd", 509, 2.0, ""))
WANTED_B = (451, 511, 513, 767, 769, 1003)
SHORT_BASES = (64, 150, 260, 371, 420, 449)   # N = 61 .. 446


def geometry(read, band=BAND, k=K):
    """(T, N, bw, B) of a DNA read as launch.cpp forms them: T = S + 1, N = kc + 1, bw = min(band / 2, N / 2), B = 2 bw + 3"""
    kc = len(read.sequence) - k + 1
    N = kc + 1
    bw = min(band // 2, N // 2)
    return len(read.signal) + 1, N, bw, 2 * bw + 3


def _case(name, read, dwell, kind):
    T, N, bw, B = geometry(read)
    return SimpleNamespace(name=name, read=read, signal=read.signal, sequence=read.sequence, T=T, N=N, bw=bw, B=B, dwell=dwell,
                           kind=kind, wide=bw > WIDE_ABOVE, fails=kind == "nan")


def read_sets(model_path):
    """(W, S): lists of cases (name, read, signal, sequence, T, N, bw, B, dwell, kind, wide, fails)"""
    _, mean, sd = synth.read_model_file(model_path)
    W = []
    for i, (name, N, dwell, kind) in enumerate(WIDE):
        r = synth.make_reads(7700 + i, 1, PORE, mean, sd, N + K - 2, dwell=dwell)[0]
        if kind == "tie":      # a homopolymer of 2 k bases in the middle: k + 1 neighbouring columns with the same parameters
            p = len(r.sequence) // 2
            r = synth.SynthRead(r.signal, r.sequence[:p] + "A" * (2 * K) + r.sequence[p + 2 * K:])
        if kind == "nan":
            s = r.signal.copy()
            s[len(s) // 2] = np.nan
            r = synth.SynthRead(s, r.sequence)
        W.append(_case(name, r, dwell, kind))
    S = [_case(f"short_{nb}", synth.make_reads(7800 + i, 1, PORE, mean, sd, nb)[0], 12.5, "") for i, nb in enumerate(SHORT_BASES)]
    return W, S


def orders(W):
    """B descending and B ascending (stable: reads of one B keep their order)"""
    return {"descending": sorted(W, key=lambda c: -c.B), "ascending": sorted(W, key=lambda c: c.B)}


def train_bar(kmers, T, num_kmers):
    """(2 m + 12) u per k-mer code, m = (columns the code labels) x (T - 1); ``kmers``: the code of lattice columns 1 .. N - 1"""
    c = np.bincount(np.asarray(kmers, dtype=np.int64), minlength=num_kmers).astype(np.float64)
    return (2.0 * c * float(T - 1) + 12.0) * U


def derived_bar_ratios(codes, w, s1, s2, ref, kmers, signal):
    """error / bar of every touched code, for a result given as parallel arrays over ``codes``: three arrays (weight, sum, sumsq)"""
    codes = np.asarray(codes, dtype=np.int64)
    bar = train_bar(kmers, len(signal) + 1, len(ref["weight"]))[codes]
    xmax = float(np.abs(signal).max())
    rw, r1, r2 = ref["weight"][codes], ref["sum"][codes], ref["sumsq"][codes]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(np.asarray(w) - rw) / (bar * np.abs(rw)), np.abs(np.asarray(s1) - r1) / (bar * rw * xmax),
                np.abs(np.asarray(s2) - r2) / (bar * np.abs(r2)))


def check_derived_bar(codes, w, s1, s2, ref, kmers, signal, what):
    """the three sums of the codes given (all with ref weight > 0) under the derived bar. Returns the worst error / bar of
    (weight, sum, sumsq)."""
    ratios = derived_bar_ratios(codes, w, s1, s2, ref, kmers, signal)
    worst = tuple(float(r.max()) for r in ratios)
    for r, key in zip(ratios, ("weight", "sum", "sumsq")):
        assert (r <= 1.0).all(), (what, key, "error / bar", worst, "code", int(np.asarray(codes)[int(np.argmax(r))]))
    return worst


def device_train(tr, i):
    """read i of a TrainBatchResult: (codes, weight, sum, sumsq)"""
    a = int(tr.em_offsets[i])
    b = a + int(tr.em_count[i])
    return tr.em_code[a:b], tr.em_weight[a:b], tr.em_sum[a:b], tr.em_sumsq[a:b]


def check_train(codes, w, s1, s2, Z, m1, e2, ref, kmers, signal, what):
    """the whole bar of this module's docstring. Returns the worst error / bar of (weight, sum, sumsq)."""
    S = len(signal)
    touched = np.flatnonzero(ref["weight"] > 0)
    assert np.array_equal(np.sort(np.asarray(codes, dtype=np.int64)), touched), (what, "touched codes differ")
    assert np.float64(Z).tobytes() == np.float64(ref["Z"]).tobytes(), (what, "Z bits", Z, ref["Z"])
    assert abs(m1 - ref["m1"]) <= 1e-8 and abs(e2 - ref["e2"]) <= 1e-8, (what, "transitions", m1, ref["m1"], e2, ref["e2"])
    assert abs(float(np.sum(w)) - S) <= 1e-8 * S, (what, "mass", float(np.sum(w)), S)
    return check_derived_bar(codes, w, s1, s2, ref, kmers, signal, what)
