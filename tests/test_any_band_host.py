"""CPU: the read sets and the train bar of tests/any_band_cases.py, before a GPU test relies on them. The sets have the widths,
dwells and row counts the diagonal any-band kernel is to be run at; the oracle at band 1 000 takes every read of them (the NaN
read as the reference takes it: without an error, with a NaN answer); the derived bar is between 16 u and 1e-9 for every k-mer
of every wide read; and the bar catches what the rtol = 1e-7 it stands beside lets through -- a k-mer's weight that lost one
lattice cell's term, and a weight moved by twice its bar."""
import numpy as np
import pytest

import any_band_cases as ab
from dynamont_amd import synth
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.usefixtures("oracle_built")


@pytest.fixture(scope="module")
def sets(models):
    return ab.read_sets(models[ab.MODEL])


@pytest.fixture(scope="module")
def orc(models, oracle_built):
    return Oracle(models[ab.MODEL], synth.PORES[ab.PORE][0], ab.BAND)


def test_read_sets_have_the_stated_geometry(sets, orc):
    W, S = sets
    assert synth.PORES[ab.PORE] == (2, False, ab.K) and orc.k == ab.K          # a DNA pore, k = 5: no polyA pad
    assert len(W) == len(ab.WIDE) == 14 and len(S) == 6
    for c, (name, N, dwell, kind) in zip(W, ab.WIDE):
        assert len(orc.kmers(c.sequence)) + 1 == c.N == N, name                # N = kc + 1, from the oracle's own k-mer count
        assert c.bw == min(ab.BAND // 2, N // 2) > ab.WIDE_ABOVE and c.B == 2 * c.bw + 3 and c.wide, name
        assert c.T == len(c.signal) + 1 >= 2 * N - 1 and c.dwell == dwell, name
        assert c.B == int(name[1:name.index("_")]), name
        # dwell 2.0: max(2, Poisson(2)) averages 2.54 samples per k-mer, the band moves every 2-3 rows; dwell 10: every ~10 rows
        assert (2.0 <= c.T / N <= 2.8) if dwell == 2.0 else (9.0 <= c.T / N <= 11.0), (name, c.T / N)
        assert c.T * c.N <= 1050 * 2750                                        # the oracle's CPU time is what a test here costs
    assert {c.B for c in W} == set(ab.WANTED_B)
    assert {(c.B, c.dwell) for c in W} >= {(451, 2.0), (451, 10.0), (511, 2.0), (511, 10.0), (513, 2.0), (513, 10.0)}
    tie = next(c for c in W if c.kind == "tie")
    km = orc.kmers(tie.sequence)
    assert "A" * (2 * ab.K) in tie.sequence and (np.diff(np.flatnonzero(km == 0)) == 1).sum() >= ab.K   # k + 1 columns in a row carry AAAAA
    nan = [c for c in W if c.kind == "nan"]
    assert len(nan) == 1 and np.isnan(nan[0].signal[len(nan[0].signal) // 2]) and np.isnan(nan[0].signal).sum() == 1 and nan[0].fails
    for c in S:
        assert len(orc.kmers(c.sequence)) + 1 == c.N < 448 and c.bw <= ab.WIDE_ABOVE and not c.wide and c.T >= 2 * c.N - 1
    o = ab.orders(W)
    assert [c.B for c in o["descending"]] == sorted((c.B for c in W), reverse=True)
    assert [c.B for c in o["ascending"]] == sorted(c.B for c in W)
    assert sorted(c.name for c in o["descending"]) == sorted(c.name for c in o["ascending"]) == sorted(c.name for c in W)
    # in both orders a workgroup that takes every second read still sees reads of another B behind each other
    for seq in o.values():
        assert len({c.B for c in seq[0::2]}) >= 3 and len({c.B for c in seq[1::2]}) >= 3


def test_oracle_takes_every_read(sets, orc):
    """... of W and S at band 1 000. The NaN read is no exception for the ORACLE: like the reference it lets NaN through its Z
    check (NT_aligner_api.cpp:288) and answers with a NaN Z; the device fails that read (tests/test_gpu_any_band.py)."""
    W, S = sets
    for c in W + S:
        a = orc.align(c.signal, c.sequence, True)
        t = orc.train(c.signal, c.sequence, dense=False)
        if c.fails:
            assert np.isnan(a["Z"]) and np.isnan(t["Z"]), c.name
            continue
        assert np.isfinite(a["Z"]) and t["Z"] == a["Z"] and len(a["signal_positions"]) == c.N - 1, c.name
        assert abs(t["weight"].sum() - len(c.signal)) <= 1e-8 * len(c.signal), c.name


def test_bar_is_between_16_u_and_1e_9(sets, orc):
    W, _ = sets
    lo, hi = np.inf, 0.0
    for c in W:
        km = orc.kmers(c.sequence)
        bar = ab.train_bar(km, c.T, orc.num_kmers)
        labelled = bar[np.unique(km)]
        assert (labelled <= 1e-9).all() and (labelled >= 16 * ab.U).all(), (c.name, labelled.max(), labelled.min())
        lo, hi = min(lo, labelled.min()), max(hi, labelled.max())
    assert ab.train_bar([3], 2, 4)[3] == 14 * ab.U and ab.train_bar([3], 3, 4)[3] == 16 * ab.U    # m = 1 is below 16 u; no read has T < 3
    assert all(c.T >= 3 for c in W)
    print(f"derived bar over W: {lo:.3g} .. {hi:.3g}")


def _cell_terms(orc, c):
    """every lattice cell's g = exp(fM + bM - Zb) + exp(fE + bE - Zb) of a read from the oracle's own rows, as (t, n, g)"""
    Wd = 2 * c.bw + 1
    fb = orc.debug_fb(c.signal, c.sequence, Wd)
    start, n_lo, n_hi = orc.bounds(c.T, c.N, c.bw)
    Zb = orc.train(c.signal, c.sequence, dense=False)["Z"]
    ts, ns, gs = [], [], []
    for t in range(1, c.T):
        a, b = max(int(n_lo[t]), 1), int(n_hi[t])
        n = np.arange(a, b)
        col = n - int(start[t])                                  # band column c + 1 <-> n = start_t + c
        with np.errstate(over="ignore", invalid="ignore"):
            g = np.exp(fb["fM"][t, col] + fb["bM"][t, col] - Zb) + np.exp(fb["fE"][t, col] + fb["bE"][t, col] - Zb)
        ts.append(np.full(len(n), t))
        ns.append(n)
        gs.append(g)
    return np.concatenate(ts), np.concatenate(ns), np.concatenate(gs)


def test_bar_rejects_a_lost_term_and_a_shift_of_twice_the_bar(sets, orc):
    """What a lost flush of the diagonal train job would look like: one cell's g missing from one k-mer's three sums. The terms
    are rebuilt from the oracle's own lattice rows; a term of 1e-8 .. 5e-8 of its k-mer's weight is taken out. rtol = 1e-7
    accepts the damaged result, the derived bar rejects it -- and it rejects every touched weight moved by twice its bar."""
    W, _ = sets
    c = W[0]
    km = orc.kmers(c.sequence).astype(np.int64)
    ref = orc.train(c.signal, c.sequence, dense=False)
    t, n, g = _cell_terms(orc, c)
    code = km[n - 1]
    x = c.signal[t - 1]
    K = orc.num_kmers
    w = np.bincount(code, weights=g, minlength=K)
    touched = np.flatnonzero(ref["weight"] > 0)
    assert np.allclose(w[touched], ref["weight"][touched], rtol=1e-11, atol=0)          # the rebuilt terms are the oracle's
    args = lambda ww, s1, s2: (touched, ww[touched], s1[touched], s2[touched], ref, km, c.signal)  # noqa: E731
    clean = ab.check_derived_bar(*args(ref["weight"], ref["sum"], ref["sumsq"]), "the oracle against itself")
    assert clean == (0.0, 0.0, 0.0)
    share = g / ref["weight"][code]
    pick = np.flatnonzero((share >= 1e-8) & (share <= 5e-8))
    assert len(pick) > 0
    j = pick[np.argmin(g[pick])]
    lost = [ref[k].copy() for k in ("weight", "sum", "sumsq")]
    lost[0][code[j]] -= g[j]
    lost[1][code[j]] -= g[j] * x[j]
    lost[2][code[j]] -= (g[j] * x[j]) * x[j]
    assert np.allclose(lost[0][touched], ref["weight"][touched], rtol=1e-7, atol=1e-9)  # today's bar lets it through
    with pytest.raises(AssertionError, match="weight"):
        ab.check_derived_bar(*args(*lost), "one term lost")
    ratios = ab.derived_bar_ratios(*args(*lost))
    assert ratios[0].max() >= 1e3 and int(touched[np.argmax(ratios[0])]) == int(code[j])   # share / bar >= 1e-8 / 1e-11
    # twice the bar, on every touched code in turn (weight) and on the sum
    bar = ab.train_bar(km, c.T, K)
    for k in touched[:: max(1, len(touched) // 16)]:
        for sign in (1.0, -1.0):
            moved = ref["weight"].copy()
            moved[k] *= 1.0 + sign * 2.0 * bar[k]
            with pytest.raises(AssertionError, match="weight"):
                ab.check_derived_bar(*args(moved, ref["sum"], ref["sumsq"]), "weight moved")
            moved = ref["sum"].copy()
            moved[k] += sign * 2.0 * bar[k] * ref["weight"][k] * float(np.abs(c.signal).max())
            with pytest.raises(AssertionError, match="sum"):
                ab.check_derived_bar(*args(ref["weight"], moved, ref["sumsq"]), "sum moved")
    # ... and the whole bar refuses other Z bits and a missing code
    full = lambda codes, Z: ab.check_train(codes, ref["weight"][codes], ref["sum"][codes], ref["sumsq"][codes], Z, ref["m1"], ref["e2"],  # noqa: E731
                                           ref, km, c.signal, "whole bar")
    assert full(touched, ref["Z"]) == (0.0, 0.0, 0.0)
    with pytest.raises(AssertionError, match="Z bits"):
        full(touched, np.nextafter(ref["Z"], 0.0))
    with pytest.raises(AssertionError, match="touched codes"):
        full(touched[1:], ref["Z"])
