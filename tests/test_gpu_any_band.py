"""GPU (-m gpu): the diagonal any-band kernel (k_band_reads<DiagonalWindow, 256, 16, ..> of band_reads.hip, without a lattice
phase and with each of the five sets of them a launch may carry: PHASES of lattice_phase.hpp) on REUSED workgroups and reads of
MIXED width. A handle created under DYN_QUEUE_CUS=2 launches two workgroups for the 14 wide reads of tests/any_band_cases.py (B = 451,
511, 513, 767, 769, 1 003; dwell 2 and 10; a structural tie; a NaN sample), so at least 12 reads run on a workgroup that has
just finished another read of another B -- what a workgroup carries over (four LDS rows initialised only up to the new B, the
arena in the previous read's layout, s_bad of a read that failed, the train job's running sums) must not reach the next read.
Held against the oracle at band 1 000 where bits or the derived train bar (any_band_cases.py) are checked, and bit for bit
against the same build at the card's own CU count everywhere."""
import numpy as np
import pytest

import any_band_cases as ab
from dynamont_amd import Aligner, synth
from oracle.pyoracle import Oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib", "oracle_built")]

ORDERS = ("descending", "ascending")
SEGMENTS = ("status", "Z", "n_segments", "seg_offsets", "signal_positions", "sequence_positions", "probabilities", "states")
TRAIN = ("status", "Z", "transitions", "trans_counts", "em_offsets", "em_count", "em_code", "em_weight", "em_sum", "em_sumsq")
PER_READ = ("status", "Z", "n_segments", "seg_offsets", "sample_dead", "transitions", "trans_counts", "em_offsets", "em_count")


@pytest.fixture(scope="module")
def sets(models):
    return ab.read_sets(models[ab.MODEL])


@pytest.fixture(scope="module")
def batches(sets):
    """order -> the batch: W in that order, then S"""
    W, S = sets
    return {name: seq + S for name, seq in ab.orders(W).items()}


@pytest.fixture(scope="module")
def want(models, sets):
    """the oracle at band 1 000, every read once per job: name -> (align(.., True), train(.., dense=False), k-mer codes)"""
    orc = Oracle(models[ab.MODEL], synth.PORES[ab.PORE][0], ab.BAND)
    W, S = sets
    return {c.name: (orc.align(c.signal, c.sequence, True), orc.train(c.signal, c.sequence, dense=False), orc.kmers(c.sequence))
            for c in W + S if not c.fails}


@pytest.fixture(scope="module")
def handles(models):
    """{2: the handle created under DYN_QUEUE_CUS=2, 0: the same build at the card's CU count}. The variable is read once, at
    the handle's creation."""
    mp = pytest.MonkeyPatch()
    mp.setenv("DYN_QUEUE_CUS", "2")
    two = Aligner(models[ab.MODEL], ab.PORE, band=ab.BAND, device=0)
    mp.delenv("DYN_QUEUE_CUS")
    mp.undo()
    free = Aligner(models[ab.MODEL], ab.PORE, band=ab.BAND, device=0)
    assert two.info.max_half_band == free.info.max_half_band == 2046
    yield {2: two, 0: free}
    two.close()
    free.close()


@pytest.fixture(scope="module")
def runs(handles, batches):
    """(job, order, cus) -> (result, arena bytes), each launched once and shared by the tests"""
    cache = {}

    def run(job, order, cus, fresh=False):
        key = (job, order, cus)
        if fresh or key not in cache:
            cases = batches[order]
            with handles[cus].batch([c.signal for c in cases], [c.sequence for c in cases]) as b:
                if job == "train":
                    b.train()
                    res = b.fetch_train()
                else:
                    b.align(job == "align")
                    res = b.fetch()
                got = (res, b.arena_bytes())
            if fresh:
                return got
            cache[key] = got
        return cache[key]
    return run


def bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


def same_bits(a, b, cols, what):
    """every column bit for bit: the per-row columns over the batch's rows, the per-read columns whole"""
    assert np.array_equal(a.seg_offsets, b.seg_offsets) if hasattr(a, "seg_offsets") else np.array_equal(a.em_offsets, b.em_offsets), what
    m = int(a.seg_offsets[-1]) if hasattr(a, "seg_offsets") else int(a.em_offsets[-1])
    for c in cols:
        x, y = getattr(a, c), getattr(b, c)
        assert x is not None and y is not None and x.shape == y.shape and x.dtype == y.dtype, (what, c)
        if x.ndim == 2:                                             # sample planes [K, cap]
            x, y = x[:, :m], y[:, :m]
        elif c not in PER_READ:                                     # per-row columns [cap]
            x, y = x[:m], y[:m]
        assert np.array_equal(bits(x), bits(y)), (what, c)


def arena_of(cases, per_cell):
    """band_arena_bytes of the largest wide read of the batch"""
    cells = max(c.T * c.B for c in cases if c.wide)
    return (cells * per_cell + 255) & ~255


def check_align_against_oracle(res, cases, want, what):
    for i, c in enumerate(cases):
        if c.fails:
            assert res.status[i] != 0 and res.n_segments[i] == 0, (what, c.name)
            continue
        assert res.status[i] == 0, (what, c.name, res.error(i))
        got, ref = res.read(i), want[c.name][0]
        assert np.array_equal(got["signal_positions"], ref["signal_positions"]), (what, c.name)
        assert np.array_equal(got["sequence_positions"], ref["sequence_positions"]), (what, c.name)
        assert got["states"] == ref["states"], (what, c.name)
        if c.wide:
            assert bits(np.float64(got["Z"])).tolist() == bits(np.float64(ref["Z"])).tolist(), (what, c.name, got["Z"], ref["Z"])
        else:
            assert abs(got["Z"] - ref["Z"]) <= 1e-9 * abs(ref["Z"]), (what, c.name)
        assert np.abs(got["probabilities"] - ref["probabilities"]).max() <= 1e-6, (what, c.name)


# ---- a. align ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_align_on_two_workgroups_equals_the_oracle_and_the_unconstrained_run(runs, batches, want, order):
    cases = batches[order]
    res, arena = runs("align", order, 2)
    base, arena_free = runs("align", order, 0)
    n_wide = sum(c.wide for c in cases)
    # two workgroups took the 14 wide reads, one arena each; the unconstrained handle gave every wide read its own
    assert n_wide == 14 and arena == 2 * arena_of(cases, 25) and arena_free == n_wide * arena_of(cases, 25)
    check_align_against_oracle(res, cases, want, f"{order}, two workgroups")
    same_bits(res, base, SEGMENTS, f"align {order}: two workgroups against the unconstrained run")


# ---- b. the failed read -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_reads_behind_the_failed_read_are_untouched_by_it(runs, batches, want, order):
    """the NaN read fails in all three jobs (s_bad is set on its workgroup); at least five wide reads stand behind it on the
    queue, of which the workgroup that took it takes some: every one of them has the oracle's answer and the unconstrained run's"""
    cases = batches[order]
    at = next(i for i, c in enumerate(cases) if c.fails)
    behind = [i for i in range(at + 1, len(cases)) if cases[i].wide]
    assert len(behind) >= 5
    al, _ = runs("align", order, 2)
    zo, _ = runs("zonly", order, 2)
    tr, _ = runs("train", order, 2)
    assert al.status[at] != 0 and zo.status[at] != 0 and tr.status[at] != 0
    assert al.status[at] == runs("align", order, 0)[0].status[at] and tr.status[at] == runs("train", order, 0)[0].status[at]
    assert al.error(at) == "Alignment failed: alignment scores do not match"
    assert tr.em_count[at] == 0
    ok = [i for i in range(len(cases)) if i != at]
    assert (al.status[ok] == 0).all() and (zo.status[ok] == 0).all() and (tr.status[ok] == 0).all()
    tr_free = runs("train", order, 0)[0]
    for i in behind:
        c = cases[i]
        ref_a, ref_t, km = want[c.name]
        for Z in (al.Z[i], zo.Z[i], tr.Z[i]):
            assert np.float64(Z).tobytes() == np.float64(ref_a["Z"]).tobytes(), (order, c.name)
        assert np.array_equal(al.read(i)["signal_positions"], ref_a["signal_positions"]), (order, c.name)
        for x, y in zip(ab.device_train(tr, i), ab.device_train(tr_free, i)):
            assert np.array_equal(bits(x), bits(y)), (order, c.name)


# ---- c. Z only --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_z_only_on_two_workgroups(runs, batches, want, order):
    cases = batches[order]
    res, arena = runs("zonly", order, 2)
    assert arena == 0                                               # nothing of the lattice is stored: no arena
    assert not res.n_segments.any()
    for i, c in enumerate(cases):
        if c.fails:
            assert res.status[i] != 0
        elif c.wide:
            assert res.status[i] == 0 and np.float64(res.Z[i]).tobytes() == np.float64(want[c.name][0]["Z"]).tobytes(), (order, c.name)
        else:
            assert res.status[i] == 0 and abs(res.Z[i] - want[c.name][0]["Z"]) <= 1e-9 * abs(want[c.name][0]["Z"]), (order, c.name)
    same_bits(res, runs("zonly", order, 0)[0], ("status", "Z", "n_segments"), f"Z only {order}")


# ---- d. the asynchronous ticket ---------------------------------------------------------------------------------------------
def test_ticket_on_two_workgroups_has_the_batch_s_bits(handles, runs, batches):
    cases = batches["descending"]
    t = handles[2].align_async(*synth.pack_reads([c.read for c in cases]), True)
    res = t.wait()
    assert t.timing()["launches"] == 1
    same_bits(res, runs("align", "descending", 2)[0], SEGMENTS, "ticket against batch, two workgroups")
    t.close()


# ---- e. train ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_train_on_two_workgroups_under_the_derived_bar_and_bit_for_bit(runs, batches, want, order):
    """Worst error / bar measured on the MI355X: profiles/any_band/train_bar.txt."""
    cases = batches[order]
    tr, arena = runs("train", order, 2)
    assert arena == 2 * arena_of(cases, 16)
    worst = np.zeros(3)
    for i, c in enumerate(cases):
        if c.fails:
            assert tr.status[i] != 0
            continue
        assert tr.status[i] == 0, (order, c.name, tr.error(i))
        _, ref, km = want[c.name]
        codes, w, s1, s2 = ab.device_train(tr, i)
        if c.wide:
            r = ab.check_train(codes, w, s1, s2, tr.Z[i], tr.transitions[3 * i], tr.transitions[3 * i + 2], ref, km, c.signal,
                               f"train {order} {c.name}")
            print(f"train, two workgroups, {order}, {c.name} (T {c.T}, B {c.B}): worst error / bar weight {r[0]:.4f} sum {r[1]:.4f} sumsq {r[2]:.4f}")
            worst = np.maximum(worst, r)
        else:   # the register sweeps' reads keep their bar
            assert abs(tr.Z[i] - ref["Z"]) <= 1e-9 * abs(ref["Z"]) and np.allclose(w, ref["weight"][codes], rtol=1e-7, atol=1e-9), (order, c.name)
    print(f"train, two workgroups, {order}: worst error / bar over the wide reads: weight {worst[0]:.4f} sum {worst[1]:.4f} sumsq {worst[2]:.4f}")
    same_bits(tr, runs("train", order, 0)[0], TRAIN, f"train {order}: two workgroups against the unconstrained run")
    again, _ = runs("train", order, 2, fresh=True)
    same_bits(tr, again, TRAIN, f"train {order}: a second run on two workgroups")


# ---- f. the riders: the five instantiations of the kernel that carry lattice phases ------------------------------------------------
RIDERS = {
    "border_confidence": (lambda al: al.set_border_confidence(8), ("border_probability", "border_window_probability"), "descending"),
    "samples": (lambda al: al.set_posterior_samples(4, 20261020), ("sample_starts", "sample_dead"), "ascending"),
    "samples_and_border": (lambda al: (al.set_posterior_samples(4, 20261020), al.set_border_confidence(8)),
                           ("sample_starts", "sample_dead", "border_probability", "border_window_probability"), "descending"),
    "border_interval": (lambda al: al.set_border_interval(0.9), ("border_lo", "border_hi", "border_mean", "border_sd"), "ascending"),
    "soft_levels": (lambda al: al.set_soft_levels(True), ("soft_weight", "soft_sum", "soft_sumsq"), "descending"),
}


@pytest.mark.parametrize("rider", list(RIDERS))
def test_rider_on_two_workgroups_has_the_unconstrained_run_s_bits(models, runs, batches, monkeypatch, rider):
    """every column the rider adds, the dead-sample counts included, every segment column and every status, the NaN read's
    among them (no rider refuses a batch for a read that fails: a failed read's rows stay empty). The riders' values against
    their yardsticks are their own tests' business; the segment columns are those of the launch without a rider."""
    switch, cols, order = RIDERS[rider]
    cases = batches[order]
    got = {}
    for cus in (2, 0):
        if cus:
            monkeypatch.setenv("DYN_QUEUE_CUS", str(cus))
        al = Aligner(models[ab.MODEL], ab.PORE, band=ab.BAND, device=0)
        if cus:
            monkeypatch.delenv("DYN_QUEUE_CUS")
        switch(al)
        with al.batch([c.signal for c in cases], [c.sequence for c in cases]) as b:
            b.align(True)
            got[cus] = (b.fetch(), b.arena_bytes())
        al.close()
    assert got[2][1] == 2 * arena_of(cases, 25) and got[0][1] == 14 * arena_of(cases, 25)
    res, base = got[2][0], got[0][0]
    at = next(i for i, c in enumerate(cases) if c.fails)
    assert res.status[at] != 0 and (np.delete(res.status, at) == 0).all()
    same_bits(res, base, SEGMENTS + cols, f"{rider} {order}: two workgroups against the unconstrained run")
    same_bits(res, runs("align", order, 2)[0], SEGMENTS, f"{rider} {order}: the segment columns with the rider against without")
    if "sample_dead" in cols:
        assert res.sample_starts.shape[0] == 4
