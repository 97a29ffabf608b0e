"""CPU: the host half of the guided band (dyn_batch_set_guide, dynamont_amd/guide.py). The guide helpers against the reference's
own band centre and hand-written move tables; every host-side refusal of the entry point with its text, on a handle without a
device; the NumPy restatement of the guided lattice (tests/guided_band_cases.py) against the CPU oracle with a diagonal guide --
which is where Z_RTOL comes from --; and the purpose, shown on the CPU first: on stalled reads the band around the fixed
diagonal at band 50 loses the borders that a window of half width 16 around the true starts finds."""
import os
import re

import numpy as np
import pytest

import band_margin_cases as bmc
import guided_band_cases as gc
from conftest import ROOT
from dynamont_amd import Aligner, _native as N, synth
from dynamont_amd import guide as G
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.usefixtures("native_lib")


# ------------------------------------------------------------------------------------------------------------- the helpers
def test_diagonal_guide_is_the_references_centre():
    """every row of reads of 2 .. 100 000 samples, T, N pairs whose products land within an ulp of an integer included"""
    pairs = [(2, 2), (3, 2), (7, 3), (90, 10), (1027, 256), (99999, 1000), (100000, 9091)]
    rng = np.random.default_rng(20261019)
    near = 0
    while near < 4:
        T, Ncol = 100001 - int(rng.integers(0, 50)), int(rng.integers(300, 2500))
        if bmc.near_integer_products(T, float(Ncol) / float(T)).size:
            pairs.append((T - 1, Ncol))
            near += 1
    pairs += [(int(rng.integers(2, 5000)), 0) for _ in range(40)]
    for S, Ncol in pairs:
        Ncol = Ncol or int(rng.integers(2, S + 2))
        T = S + 1
        ratio = float(Ncol) / float(T)
        g = G.diagonal_guide(S, Ncol)
        assert g.dtype == np.int32 and g.shape == (S,)
        if S <= 5000:
            assert g.tolist() == [bmc.mid(t, ratio) for t in range(1, T)], (S, Ncol)
        else:
            for t in list(range(1, 200)) + bmc.near_integer_products(T, ratio).tolist() + [T - 2, T - 1] + rng.integers(1, T, 2000).tolist():
                assert int(g[t - 1]) == bmc.mid(int(t), ratio), (S, Ncol, t)
        assert (np.diff(g) >= 0).all() and g[-1] <= Ncol - 1


def test_the_diagonal_guide_is_the_oracles_band(models):
    orc = Oracle(models["syn5"], 0)
    for T, Ncol in [(90, 10), (300, 40), (1027, 256), (2000, 333)]:
        start, _, _ = orc.bounds(T, Ncol, 7)
        assert (G.diagonal_guide(T - 1, Ncol) - 7).tolist() == start[1:].tolist()


def test_guide_from_starts():
    g = G.guide_from_starts([0, 3, 3, 10], 8, 5)                  # two columns begin at sample 3; the last start is past the end
    assert g.tolist() == [1, 1, 1, 3, 3, 3, 3, 3] and g.dtype == np.int32
    assert G.guide_from_starts([2, 4], 6, 3).tolist() == [0, 0, 1, 1, 2, 2]          # column 0 until the first start
    assert G.guide_from_starts([0, 1, 2, 3, 4], 6, 3).tolist() == [1, 2, 2, 2, 2, 2]  # clamped to N - 1
    assert G.guide_from_starts([], 3, 2).tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="non-decreasing"):
        G.guide_from_starts([4, 2], 6, 3)


def test_guide_from_moves_on_hand_written_tables():
    # stride 5, k = 3 (centre base j + 1): bases start at blocks 0, 1, 3, 4, 7 -> samples 0, 5, 15, 20, 35
    mv = [5, 1, 1, 0, 1, 1, 0, 0, 1]
    assert G.base_starts_from_moves(mv).tolist() == [0, 5, 15, 20, 35]
    g = G.guide_from_moves(mv, 40, 5, 3)                           # k-mers 0, 1, 2 start with bases 1, 2, 3: samples 5, 15, 20
    assert g.tolist() == [0] * 5 + [1] * 10 + [2] * 5 + [3] * 20
    # ts > 0: the table begins 7 samples into the aligner's signal
    g = G.guide_from_moves(mv, 40, 5, 3, ts=7)
    assert g.tolist() == [0] * 12 + [1] * 10 + [2] * 5 + [3] * 13
    # stride 6, k = 5 (centre base j + 2), a stall of 40 zero flags between bases 3 and 4
    mv6 = [6, 1, 1, 1, 1] + [0] * 40 + [1, 1, 1]
    st = G.base_starts_from_moves(mv6)
    assert st.tolist() == [0, 6, 12, 18, 264, 270, 276]
    g = G.guide_from_moves(mv6, 290, 7, 5)                         # k-mers 0, 1, 2 <- bases 2, 3, 4: samples 12, 18, 264
    assert g.tolist() == [0] * 12 + [1] * 6 + [2] * 246 + [3] * 26
    # starts past the last sample never count
    assert G.guide_from_moves(mv6, 100, 7, 5).tolist() == [0] * 12 + [1] * 6 + [2] * 82
    # reverse: base b is move n - 1 - b and begins, in reversed samples, where that move ended
    g = G.guide_from_moves(mv, 40, 5, 3, reverse=True)             # ends 5, 15, 20, 35, 40 -> reversed starts 0, 5, 20, 25, 35
    assert g.tolist() == [0] * 5 + [1] * 15 + [2] * 5 + [3] * 15
    # more bases than moves (a prepended pad): the two leading extra bases take the first move's start -- base starts 0, 0, 0, 5,
    # 15, 20, 35, k-mers 0 .. 4 <- bases 1 .. 5: samples 0, 0, 5, 15, 20
    assert G.guide_from_moves(mv, 40, 7, 3).tolist() == [2] * 5 + [3] * 10 + [4] * 5 + [5] * 20
    with pytest.raises(ValueError):
        G.guide_from_moves([5, 0, 0], 10, 5, 3)
    with pytest.raises(ValueError):
        G.guide_from_moves(mv, 40, 2, 3)


def test_synthetic_move_table_follows_the_true_starts(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    for r in gc.build_reads(mean, sd)["stall_mv"]:
        mv, ts = gc.moves_over_starts(r.starts, len(r.signal))
        assert int(mv[0]) == 5 and int((mv[1:] != 0).sum()) == r.n_kmers + gc.K - 1
        g = G.guide_from_moves(mv, len(r.signal), len(r.sequence), gc.K, ts=ts)
        assert np.abs(g.astype(int) - gc.true_guide(r).astype(int)).max() <= 4   # a block holds one move: a few columns of lag


# ------------------------------------------------------------------------------------------ validation on a host-only handle
def _host_batch(al, reads):
    sig = [r.signal for r in reads]
    return al.batch(sig, [r.sequence for r in reads])


def test_symbol_header_and_abi(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION 10\b", hdr)
    assert re.search(r"int dyn_batch_set_guide\(dyn_batch\* b, const int32_t\* centres, uint64_t count, uint32_t half_width\);", hdr)
    assert "dyn_batch_set_guide" in N.SIGNATURES and getattr(native_lib, "dyn_batch_set_guide") is not None
    assert {"band_reads.hip", "guided_band.hip"} <= set(N.SOURCES) and {"band_reads.hpp", "guided_band_kernels.hpp", "border_kernels.hpp"} <= set(N.HEADERS)
    assert native_lib.dyn_batch_set_guide(None, None, 0, 8) == N.DYN_ERR_INVALID_ARGUMENT
    assert re.search(r"int dyn_batch_arena_bytes\(const dyn_batch\* b, uint64_t\* bytes\);", hdr) and "dyn_batch_arena_bytes" in N.SIGNATURES
    assert native_lib.dyn_batch_arena_bytes(None, None) == N.DYN_ERR_INVALID_ARGUMENT


def test_every_refusal_with_its_text(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    reads = gc.build_reads(mean, sd)["b"][:3]
    al = Aligner(models["syn5"], gc.PORE, band=50, device="host")
    guides = [gc.diagonal(r) for r in reads]
    flat = np.concatenate(guides)
    off = np.concatenate([[0], np.cumsum([len(g) for g in guides])])
    n_last = [r.n_kmers for r in reads]                            # N - 1
    with _host_batch(al, reads) as b:
        with pytest.raises(ValueError, match=r"dyn_batch_set_guide: count %d differs from the batch's %d samples" % (len(flat) - 1, len(flat))):
            b.set_guide(flat[:-1], 8)
        for hw in (0, 2047, 100000):
            with pytest.raises(ValueError, match=r"dyn_batch_set_guide: half_width %d is outside \[1, 2046\]" % hw):
                b.set_guide(flat, hw)
        bad = flat.copy()
        bad[off[1] + 17] = n_last[1] + 1
        with pytest.raises(ValueError, match=r"read 1, sample 17: centre %d is outside \[0, %d\]" % (n_last[1] + 1, n_last[1])):
            b.set_guide(bad, 8)
        bad = flat.copy()
        bad[off[2] + 5] = -1
        with pytest.raises(ValueError, match=r"read 2, sample 5: centre -1 is outside \[0, %d\]" % n_last[2]):
            b.set_guide(bad, 8)
        bad = flat.copy()
        s = int(np.flatnonzero(np.diff(guides[0]) > 0)[3]) + 1     # a sample where the guide has just stepped up
        bad[s + 1] = bad[s] - 1
        with pytest.raises(ValueError, match=r"read 0, sample %d: centre %d is below the previous sample's %d" % (s + 1, bad[s + 1], bad[s])):
            b.set_guide(bad, 8)
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):   # unguided: the job needs the device, as ever
            b.train()
        b.set_guide(flat, 8)                                       # a valid guide is accepted (validated; no device to copy to)
        b.set_guide(flat, 2046)
        assert b.arena_bytes() == 0
        with pytest.raises(ValueError, match="dyn_batch_train: the batch carries a guide .* training inside a guided band is not supported"):
            b.train()
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            b.align(True)
    # a read that fails validation has no lattice: its samples are not checked, the others are
    with al.batch([reads[0].signal, np.zeros(30)], [reads[0].sequence, "ACG"]) as b:
        b.set_guide(np.concatenate([guides[0], np.full(30, 12345, dtype=np.int32)]), 4)
    with pytest.raises(ValueError, match="signals and guides differ"):
        al.align_batch_guided([reads[0].signal], [reads[0].sequence], [], 4)
    with pytest.raises(ValueError, match="guide 0 holds 3 entries"):
        al.align_batch_guided([reads[0].signal], [reads[0].sequence], [np.zeros(3, dtype=np.int32)], 4)
    al.close()


# ------------------------------------------------------------------------------------------- the restatement and the oracle
@pytest.fixture(scope="module")
def ctx(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    al = Aligner(models["syn5"], gc.PORE, device="host")
    assert al.info.log_e1 == 0.0                                   # the model (and the kernel) add 0.0 for it
    c = dict(fam=gc.build_reads(mean, sd), m1=float(al.info.log_m1), e2=float(al.info.log_e2), model=models["syn5"],
             pore=synth.PORES[gc.PORE][0])
    al.close()
    return c


def model_of(ctx, orc, r, guide, hw):
    km = orc.kmers(r.sequence)
    mean, sd = orc.table()
    return gc.model_align(r.signal, mean[km], sd[km], ctx["m1"], ctx["e2"], guide, hw)


FAMILY_BAND = {"a": 50, "a2": 270, "b": 4093, "stall": 50, "stall_mv": 50, "e": 16}


def test_restatement_equals_the_oracle_with_a_diagonal_guide(ctx):
    """borders equal; the largest |Z_model - Z_oracle| / |Z_oracle| is what Z_RTOL is eight times of, every read of every
    family (w apart: one read of 4 100 k-mers, too large for the model's whole-lattice arrays)"""
    worst = 0.0
    for name, band in FAMILY_BAND.items():
        orc = Oracle(ctx["model"], ctx["pore"], band)
        dev = 0.0
        for r in ctx["fam"][name]:
            Ncol = r.n_kmers + 1
            mo = model_of(ctx, orc, r, gc.diagonal(r), min(band // 2, Ncol // 2))
            ref = orc.align(r.signal, r.sequence, True)
            assert mo.ok and np.array_equal(mo.signal_positions, ref["signal_positions"].astype(np.int64)), name
            assert np.abs(mo.probabilities - ref["probabilities"]).max() <= 1e-12
            dev = max(dev, abs(mo.Z - ref["Z"]) / abs(ref["Z"]))
        print("family %-8s max |Z_model - Z_oracle| / |Z_oracle| = %.3g" % (name, dev))
        worst = max(worst, dev)
    print("all families: %.3g; Z_RTOL = %.3g" % (worst, gc.Z_RTOL))
    assert worst <= gc.Z_RTOL                                      # (the constant is 8 x the maximum measured when it was set)


def test_the_purpose_on_the_cpu(ctx):
    """the stall family: covers() holds, so oracle(band 4093) -- whose band is then the whole lattice -- is the truth; the band
    around the diagonal at band 50 misses it on every read, the window of half width 16 around the true starts finds it"""
    reads = ctx["fam"]["stall"]
    assert len(reads) >= 12 and all(60 <= r.n_kmers <= 150 for r in reads)
    o50, o_all = Oracle(ctx["model"], ctx["pore"], gc.STALL_BAND), Oracle(ctx["model"], ctx["pore"], 4093)
    for i, r in enumerate(reads):
        T, Ncol = len(r.signal) + 1, r.n_kmers + 1
        stall = int(np.diff(np.append(r.starts, len(r.signal))).max())
        assert 0.29 <= stall / len(r.signal) <= 0.51 and gc.covers(T, Ncol), i
        truth = o_all.align(r.signal, r.sequence, True)["signal_positions"].astype(np.int64)
        narrow = o50.align(r.signal, r.sequence, True)["signal_positions"].astype(np.int64)
        assert not np.array_equal(narrow, truth), i
        mo = model_of(ctx, o_all, r, gc.true_guide(r), gc.STALL_HALF_WIDTH)
        assert mo.ok and np.array_equal(mo.signal_positions, truth), i


def test_covers_agrees_with_a_full_lattice_model(ctx):
    """where covers() holds, the model with a window that spans every column gives the oracle's Z at band 4093 to Z_RTOL and its
    borders; covers() itself turns false between T = 3.8 N and 4.1 N"""
    o_all = Oracle(ctx["model"], ctx["pore"], 4093)
    for r in ctx["fam"]["b"][:4]:
        Ncol = r.n_kmers + 1
        mo = model_of(ctx, o_all, r, gc.random_staircase(np.random.default_rng(r.n_kmers), len(r.signal), Ncol), Ncol)
        ref = o_all.align(r.signal, r.sequence, True)
        assert mo.ok and np.array_equal(mo.signal_positions, ref["signal_positions"].astype(np.int64))
        assert abs(mo.Z - ref["Z"]) <= gc.Z_RTOL * abs(ref["Z"])
    assert gc.covers(380, 100) and not gc.covers(410, 100) and gc.covers(200, 100)


def test_guided_margin_restatement():
    """with a diagonal guide the guided margin is the band margin's definition (tests/band_margin_cases.py)"""
    rng = np.random.default_rng(5)
    for k in range(300):
        T = int(rng.integers(3, 160))
        Ncol = int(rng.integers(2, T // 2 + 2))
        bw = min(int(rng.integers(1, 30)), Ncol // 2)
        ratio = float(Ncol) / float(T)
        if 2 * (Ncol - 1) > T - 1:
            continue
        segrow = bmc.make_path(T, Ncol, bw, ratio, ("low", "high", "random")[k % 3], rng)
        assert gc.guided_margin(segrow, T, Ncol, G.diagonal_guide(T - 1, Ncol), bw) == bmc.brute(segrow, T, Ncol, bw, ratio)
    # a guide shifted by exactly the half width under a path: slack 0 on every row where that edge is real
    segrow = np.arange(1, 60, 2)
    path = np.searchsorted(segrow, np.arange(1, 70), side="right")
    low, high, edge = gc.guided_margin(segrow, 70, 31, np.clip(path + 4, 0, 30), 4)
    assert low == 0 and edge == int(((np.clip(path + 4, 0, 30) - 4 >= 2) & (np.clip(path + 4, 0, 30) - 4 == path)).sum()) and high > 0
