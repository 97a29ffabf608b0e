"""CPU: what a job takes from the handle's opt-in switches at its submission, pinned on a handle without a device.
  1. every unordered pair of the eight switches (rescale, border confidence, border interval, posterior samples, auto-guide, guide
     rescue, event stats, segment scores) through ``Batch.align`` and through ``Aligner.align_async``: the pairs that do not combine
     are refused with their literal text, every other pair -- and every pair of a Z-only job -- gets as far as "no GPU bound to
     this handle"
  2. a batch that carries a guide (``Batch.set_guide``) against the five switches it does not combine with
  3. the Python record of a job's switches: all off for a Z-only job and for a batch never aligned, which fetches nothing optional
GPU (-m gpu), at the end: the members of a MERGED launch -- event stats and segment scores on for all, band margins for some --
fetch the columns a synchronous batch of the same reads gives, bit for bit.
(What the jobs compute needs a device: the tests/test_gpu_*.py file of each switch.)"""
import itertools

import numpy as np
import pytest

from dynamont_amd import Aligner, _native as N, guide as G, synth
from dynamont_amd._dynamont import AlignBatchResult, JobWants, _OPTIONAL

pytestmark = pytest.mark.usefixtures("native_lib")

PORE, K = "dna_r9", 5  # k = 5 on conftest's "syn5" table, no polyA pad

# name -> (switch on, switch off, the setter, how a refusal names the switch when it is the OTHER one)
SWITCHES = {
    "rescale": (lambda al: al.set_rescale(2), lambda al: al.set_rescale(0), "dyn_aligner_set_rescale", "(a, iters > 0)"),
    "confidence": (lambda al: al.set_border_confidence(8), lambda al: al.set_border_confidence(0),
                   "dyn_aligner_set_border_confidence", "(a, window > 0)"),
    "interval": (lambda al: al.set_border_interval(0.9), lambda al: al.set_border_interval(0.0),
                 "dyn_aligner_set_border_interval", "(a, mass > 0)"),
    "samples": (lambda al: al.set_posterior_samples(4, 11), lambda al: al.set_posterior_samples(0),
                "dyn_aligner_set_posterior_samples", "(a, count > 0)"),
    "auto_guide": (lambda al: al.set_auto_guide(16), lambda al: al.set_auto_guide(0), "dyn_aligner_set_auto_guide", "(a, half_width > 0)"),
    "rescue": (lambda al: al.set_guide_rescue(1, 16), lambda al: al.set_guide_rescue(0, 0),
               "dyn_aligner_set_guide_rescue", "(a, half_width > 0)"),
    "event_stats": (lambda al: al.set_event_stats(True), lambda al: al.set_event_stats(False), "dyn_aligner_set_event_stats", "(a, 1)"),
    "scores": (lambda al: al.set_segment_scores(8), lambda al: al.set_segment_scores(0),
               "dyn_aligner_set_segment_scores", "(a, window > 0)"),
}
# the pairs a synchronous align(calc_probabilities = 1) job refuses: (the switch the text says "is on", the one it "does not combine with")
SYNC_REFUSALS = [("samples", "rescale"), ("rescue", "rescale"), ("interval", "confidence"), ("rescue", "confidence"),
                 ("interval", "samples"), ("interval", "auto_guide"), ("interval", "rescue"), ("samples", "auto_guide"),
                 ("samples", "rescue"), ("rescue", "auto_guide")]
# a ticket is refused for these too: the auto-guide is the tickets' switch
ASYNC_REFUSALS = SYNC_REFUSALS + [("auto_guide", "rescale"), ("auto_guide", "confidence")]
NO_GPU = "no GPU bound to this handle"


def refusal(api, on, other):
    return "%s: %s is on, which does not combine with %s%s" % (api, SWITCHES[on][2], SWITCHES[other][2], SWITCHES[other][3])


@pytest.fixture(scope="module")
def host(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    reads = synth.make_reads(4401, 3, PORE, mean, sd, (20, 40))
    al = Aligner(models["syn5"], PORE, device="host")
    yield al, reads
    al.close()


def outcome(call):
    """(exception class, message) of a call that must not get through on a handle without a device"""
    with pytest.raises((ValueError, RuntimeError)) as e:
        call()
    return type(e.value), str(e.value)


def test_every_pair_of_switches_sync_and_async(host):
    al, reads = host
    want = {frozenset(p): p for p in SYNC_REFUSALS}
    want_async = {frozenset(p): p for p in ASYNC_REFUSALS}
    assert (len(want), len(want_async)) == (10, 12)
    pairs = list(itertools.combinations(SWITCHES, 2))
    assert len(pairs) == 28
    pk = synth.pack_reads(reads)
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        for x, y in pairs:
            SWITCHES[x][0](al)
            SWITCHES[y][0](al)
            try:
                for api, table, run in (("dyn_batch_align", want, b.align), ("dyn_batch_align_async", want_async, lambda calc: al.align_async(*pk, calc))):
                    kind, msg = outcome(lambda: run(True))
                    if frozenset((x, y)) in table:
                        assert (kind, msg) == (ValueError, refusal(api, *table[frozenset((x, y))])), (api, x, y)
                    else:
                        assert kind is RuntimeError and NO_GPU in msg, (api, x, y, msg)
                    kind, msg = outcome(lambda: run(False))                # the Z-only job reads none of the switches
                    assert kind is RuntimeError and NO_GPU in msg, (api, x, y, msg)
            finally:
                SWITCHES[x][1](al)
                SWITCHES[y][1](al)
        kind, msg = outcome(lambda: b.align(True))                         # everything off again: nothing left to refuse
        assert kind is RuntimeError and NO_GPU in msg


def test_a_guided_batch_against_the_switches(host):
    al, reads = host
    carries = "dyn_batch_align: the batch carries a guide "
    texts = {"rescale": carries + "(dyn_batch_set_guide), which does not combine with dyn_aligner_set_rescale(a, iters > 0)",
             "confidence": carries + "(dyn_batch_set_guide), which does not combine with dyn_aligner_set_border_confidence(a, window > 0)",
             "samples": carries + "(dyn_batch_set_guide / dyn_batch_auto_guide), which does not combine with "
                                  "dyn_aligner_set_posterior_samples(a, count > 0)",
             "interval": carries + "(dyn_batch_set_guide / dyn_batch_auto_guide), which does not combine with "
                                   "dyn_aligner_set_border_interval(a, mass > 0)",
             "rescue": "dyn_batch_align: dyn_aligner_set_guide_rescue is on and the batch carries a guide (dyn_batch_set_guide / "
                       "dyn_batch_auto_guide); a guided batch is not rescued"}
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        b.set_guide(np.concatenate([G.diagonal_guide(len(r.signal), len(r.sequence) - K + 2) for r in reads]), 8)
        for name, text in texts.items():
            SWITCHES[name][0](al)
            try:
                assert outcome(lambda: b.align(True)) == (ValueError, text), name
                kind, msg = outcome(lambda: b.align(False))
                if name in ("rescale", "confidence"):                      # these two are refused for the Z-only job of a guided batch too
                    assert (kind, msg) == (ValueError, text), name
                else:
                    assert kind is RuntimeError and NO_GPU in msg, (name, msg)
            finally:
                SWITCHES[name][1](al)
        for name in ("event_stats", "scores", "auto_guide"):               # a guided batch takes these (auto-guide is the tickets' switch)
            SWITCHES[name][0](al)
            try:
                kind, msg = outcome(lambda: b.align(True))
                assert kind is RuntimeError and NO_GPU in msg, (name, msg)
            finally:
                SWITCHES[name][1](al)


def test_the_record_of_a_job(host):
    al, reads = host
    assert JobWants() == JobWants(False, False, False, False, 0, False, False, False, None) and not any(JobWants())
    assert set(_OPTIONAL) == set(JobWants._fields) - {"auto_guide"}
    for name in SWITCHES:
        SWITCHES[name][0](al)
    try:
        off = np.arange(4, dtype=np.uint64)
        assert al._job_wants(False) == JobWants() and al._job_wants(False, off) == JobWants()   # calc_probabilities = False: all off
        w = al._job_wants(True)
        assert (w.levels, w.rescale, w.scores, w.borders, w.samples, w.intervals, w.margins, w.rescue, w.auto_guide) == \
            (True, True, True, True, 4, True, False, True, None)           # (a synchronous batch is not auto-guided)
        t = al._job_wants(True, off)
        assert t.auto_guide[0] == 8 and t.auto_guide[1] is off and t[:-1] == w[:-1]
    finally:
        for name in SWITCHES:
            SWITCHES[name][1](al)
    assert al._job_wants(True, off) == JobWants()
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        assert b._wants == JobWants()                                      # never aligned
        res = AlignBatchResult(b.n, b.capacity)
        res.level_mean = res.rescue = res.guide_rounds = res.band_used = np.zeros(1)   # what an earlier job may have left
        res._fetch_optional(N.lib(), b._h, al, b._wants)                   # no native call: none could succeed on this handle
        for cols, _, _ in _OPTIONAL.values():
            assert all(getattr(res, attr) is None for attr, _, _ in cols)
        assert res.band_used is None


# ---- GPU: the members of a merged launch ---------------------------------------------------------------------------------------------
def _bits(res, attr, count):
    return np.ascontiguousarray(getattr(res, attr)[:count]).view(np.uint8)


@pytest.mark.gpu
def test_members_of_a_merged_launch_fetch_their_own_columns(models):
    """Six tickets of 3-4 reads (60-120 samples each) submitted behind one that keeps the GPU busy, so that they wait together and
    share launches; event stats and segment scores on for all, band margins on for every second one. Every member's levels, scores
    and margins equal, bit for bit, those of a synchronous batch of its reads; a member that did not ask for margins is refused."""
    _, mean, sd = synth.read_model_file(models["syn5"])
    small = [synth.make_reads(4430 + j, 3 + j % 2, PORE, mean, sd, (26, 36), dwell=3.0) for j in range(6)]
    assert all(60 <= len(r.signal) <= 120 for reads in small for r in reads)
    busy = synth.pack_reads(synth.make_reads(4429, 300, PORE, mean, sd, (300, 500)))
    al = Aligner(models["syn5"], PORE, device=0)
    try:
        al.set_event_stats(True)
        al.set_segment_scores(4)
        al.set_band_margin(True)
        want = [al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True) for reads in small]
        packed = [synth.pack_reads(reads) for reads in small]
        for attempt in range(3):   # (whether tickets meet in the queue is a matter of timing, as in tests/test_gpu_async.py)
            first = al.align_async(*busy, True)
            tickets = []
            for j, pk in enumerate(packed):
                al.set_band_margin(j % 2 == 0)
                tickets.append(al.align_async(*pk, True))
            first.wait()
            shares = []
            for j, (t, w) in enumerate(zip(tickets, want)):
                got = t.wait()
                total = int(w.seg_offsets[w.n])
                assert np.array_equal(got.seg_offsets, w.seg_offsets) and np.array_equal(got.signal_positions[:total], w.signal_positions[:total])
                for attr in ("level_mean", "level_stdv", "level_median", "median_delta", "mad_delta", "homogeneity"):
                    assert np.array_equal(_bits(got, attr, total), _bits(w, attr, total)), (j, attr)
                if j % 2 == 0:
                    for attr in ("band_margin_low", "band_margin_high", "band_edge_rows"):
                        assert np.array_equal(getattr(got, attr), getattr(w, attr)), (j, attr)
                else:
                    assert got.band_margin_low is None
                    m = np.zeros(3 * t.n, dtype=np.uint32)
                    out = N.DynBandMarginOut(*(m[k * t.n:].ctypes.data_as(N.c_u32_p) for k in range(3)), t.n)
                    with pytest.raises(ValueError) as e:
                        t.fetch_band_margin(out)
                    assert str(e.value) == "dyn_batch_fetch_band_margin: the batch was submitted without dyn_aligner_set_band_margin(a, 1)"
                shares.append(t.timing()["launch_share"])
            for t in tickets + [first]:
                t.close()
            if sum(1 for x in shares if x < 1.0) >= 2:
                break
        assert sum(1 for x in shares if x < 1.0) >= 2, shares              # at least one launch was shared
    finally:
        al.close()
