"""Shared by tests/test_guided_train_host.py and tests/test_gpu_guided_train.py (no GPU, no library): guided-band training
(dyn_batch_train_guided) restated in plain NumPy float64 -- the forward and backward sweeps of
tests/guided_band_cases.py inside the guided window, then per cell g = exp(LPM) + exp(LPE), summed per lattice column in
ascending t into (w, s1 = sum g x, s2 = sum (g x) x) with x = signal[t - 1], and grouped by k-mer code, columns in ascending
order (the host finalisation's order) -- and the comparison bar of a training result against ``Oracle.train(..., dense=False)``.

The bar (``check_against_oracle``):
  touched codes (weight > 0) equal as sets;
  weight   np.allclose(rtol=1e-7, atol=1e-12): the project's bar for the wide-band kernel (tests/fuzz_wide_band.py);
  sumsq    the same rtol / atol (its terms are all >= 0, as the weight's are);
  sum      |d| <= 1e-7 * weight_ref * max|x| + 1e-12: signed terms can cancel, so the weight's bar is carried through the sum;
  sum(weight) within 1e-8 * S of S (S samples: every row's posterior mass is 1);
  m1 / e2  within 1e-8.

Largest deviations observed (printed by the tests, -s), each as the multiple of its own bar's scale the worst k-mer reached
(weight: |d| / (|w_ref| + atol / rtol); sum: |d| / (w_ref max|x| + atol / rtol); sumsq like weight), then |sum(weight) - S| / S:
  CPU, the restatement vs the oracle (tests/test_guided_train_host.py)
    family a, diagonal, band 50 (24 reads)        8.9e-15  4.3e-15  8.4e-15   7.0e-12
    family a2, diagonal, band 270 (4 reads)       1.1e-13  8.7e-14  1.1e-13   3.1e-12
    family b, random staircases, band 4093 (16)   5.7e-14  2.5e-14  5.7e-14   4.6e-13
    stall, true starts, half width 16 (16)        3.7e-16  1.4e-16  7.5e-16   2.5e-13
    stall_mv, move table, half width 16 (6)       1.1e-14  3.6e-15  1.1e-14   2.2e-12
  MI355X, the device vs the oracle (tests/test_gpu_guided_train.py; the device runs the reference's own exp / log1p, the
  restatement NumPy's, which is why the device sits closer to the oracle than the restatement does)
    a at half widths 25 / 32 / 100 / 126 (8 each) 9.0e-16  1.8e-16  6.7e-16   7.0e-12
    a2 at half width 135 (4)                      6.4e-16  2.0e-16  6.2e-16   3.1e-12
    w at half width 2046 (1)                      4.3e-16  1.4e-16  4.1e-16   3.8e-12
    b, diagonal / true / random (16 each)         3.9e-16  1.1e-16  3.8e-16   4.6e-13
    stall / stall_mv vs oracle(4093) (16 / 6)     6.8e-16  1.8e-16  7.5e-16   2.2e-12
    stall / stall_mv / e vs the restatement       1.1e-14  3.6e-15  1.1e-14   2.2e-12
  -- eight orders inside the 1e-7 bar on the weights, four inside the 1e-8 bar on the mass.
"""
from types import SimpleNamespace

import numpy as np

import guided_band_cases as gc

RTOL, ATOL = 1e-7, 1e-12


def model_train(signal, kmers, mean, sd, log_m1, log_e2, guide, hw):
    """kmers: the k-mer code of lattice columns 1 .. N-1 (entry n - 1); mean / sd: their emission parameters. Returns ok (the
    reference's Z check), Z (= Zb), Zf, the per-column sums col_w / col_s1 / col_s2 (entry n - 1), the per-code sums as a dict
    code -> (w, s1, s2) over codes with w > 0, and the transition estimates m1 / e2."""
    x = np.asarray(signal, dtype=np.float64)
    kmers = np.asarray(kmers, dtype=np.int64)
    T, N = len(x) + 1, len(mean) + 1
    hw = int(hw)
    B = 2 * hw + 3
    c = gc.centres(guide, T)
    lo_b = np.maximum(c - hw, 0)
    lo_f = np.maximum(c - hw, 1)
    hi = np.minimum(c + hw + 1, N)
    score = gc.log_normal_pdf(x[:, None], np.asarray(mean)[None, :], np.asarray(sd)[None, :])
    NEG = gc.NEG
    with np.errstate(invalid="ignore", over="ignore"):
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
            up = n + 1 < N
            ext[up] = (bM[t + 1, n[up] + 1] + score[t, n[up]]) + log_m1
            st = n > 0
            e_next = bE[t + 1, n[st]]
            sc = score[t, n[st] - 1]
            bM[t, n[st]] = e_next + sc
            ext[st] = gc.log_plus(ext[st], (e_next + sc) + log_e2)
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
            fE[t, a:b] = gc.log_plus((fM[t - 1, n] + sc) + 0.0, (fE[t - 1, n] + sc) + log_e2)
        Zf = fE[T - 1, N - 1]
        ok = bool(np.isfinite(Zf) and np.isfinite(Zb) and not abs(Zf - Zb) / float(T * B) > 1e-8)
        out = SimpleNamespace(ok=ok, Z=float(Zb), Zf=float(Zf), T=T, N=N)
        if not ok:
            return out
        col_w, col_s1, col_s2 = np.zeros(N - 1), np.zeros(N - 1), np.zeros(N - 1)
        for t in range(1, T):                                   # ascending t: the order of the kernel's per-row update
            a, b = int(lo_f[t]), int(hi[t])
            if a >= b:
                continue
            LPM = (fM[t, a:b] + bM[t, a:b]) - Zb
            LPE = (fE[t, a:b] + bE[t, a:b]) - Zb
            g = np.exp(LPM) + np.exp(LPE)
            xt = x[t - 1]
            col_w[a - 1:b - 1] += g
            col_s1[a - 1:b - 1] += g * xt
            col_s2[a - 1:b - 1] += (g * xt) * xt
    codes = {}
    for code in np.unique(kmers):
        w = s1 = s2 = 0.0
        for n in np.flatnonzero(kmers == code):                 # columns in ascending order
            w += col_w[n]
            s1 += col_s1[n]
            s2 += col_s2[n]
        if w > 0.0:
            codes[int(code)] = (w, s1, s2)
    out.col_w, out.col_s1, out.col_s2, out.codes = col_w, col_s1, col_s2, codes
    sm, se = float(N - 1), float(T - 1 - 2 * (N - 1))
    out.m1, out.e2 = sm / (sm + se), se / (sm + se)
    return out


def dense(codes, num_kmers):
    """code -> (w, s1, s2) as three dense arrays"""
    w, s1, s2 = np.zeros(num_kmers), np.zeros(num_kmers), np.zeros(num_kmers)
    for c, (a, b, d) in codes.items():
        w[c], s1[c], s2[c] = a, b, d
    return w, s1, s2


def device_codes(res, i):
    """read i of a TrainBatchResult as code -> (w, s1, s2)"""
    a = int(res.em_offsets[i])
    b = a + int(res.em_count[i])
    return {int(c): (float(w), float(s1), float(s2)) for c, w, s1, s2 in zip(res.em_code[a:b], res.em_weight[a:b], res.em_sum[a:b], res.em_sumsq[a:b])}


def check_against_oracle(codes, m1, e2, ref, signal, what):
    """the bar of this module's docstring; ``ref`` = Oracle.train(..., dense=False). Returns the largest deviations seen, each
    relative to its own bar's scale: (weight, sum, sumsq, |sum(weight) - S| / S)."""
    S = len(signal)
    xmax = float(np.abs(signal).max())
    touched = np.flatnonzero(ref["weight"] > 0)
    assert sorted(codes) == touched.tolist(), (what, "touched codes differ")
    w = np.array([codes[c][0] for c in touched])
    s1 = np.array([codes[c][1] for c in touched])
    s2 = np.array([codes[c][2] for c in touched])
    rw, r1, r2 = ref["weight"][touched], ref["sum"][touched], ref["sumsq"][touched]
    dev = (float((np.abs(w - rw) / (RTOL * np.abs(rw) + ATOL)).max()) * RTOL,
           float((np.abs(s1 - r1) / (RTOL * rw * xmax + ATOL)).max()) * RTOL,
           float((np.abs(s2 - r2) / (RTOL * np.abs(r2) + ATOL)).max()) * RTOL,
           abs(float(w.sum()) - S) / S)
    assert np.allclose(w, rw, rtol=RTOL, atol=ATOL), (what, "weight", dev)
    assert np.allclose(s2, r2, rtol=RTOL, atol=ATOL), (what, "sumsq", dev)
    assert (np.abs(s1 - r1) <= RTOL * rw * xmax + ATOL).all(), (what, "sum", dev)
    assert abs(float(w.sum()) - S) <= 1e-8 * S, (what, "mass", dev)
    assert abs(m1 - ref["m1"]) <= 1e-8 and abs(e2 - ref["e2"]) <= 1e-8, (what, "transitions", m1, ref["m1"], e2, ref["e2"])
    return dev


def weight_shift(w_a, w_b, S):
    """sum_k |w_a[k] - w_b[k]| / S: the share of a read's posterior mass that lies on other k-mers"""
    return float(np.abs(np.asarray(w_a) - np.asarray(w_b)).sum()) / float(S)
