"""GPU (-m gpu): the per-k-mer level summary (Aligner.set_kmer_summary, kmer_summary.hip). All six integers of every k-mer and
the four totals must EQUAL the Python-int restatement of the definition (tests/kmer_summary_cases.py):
  1. the product's kernels on path arrays of the test's own (tests/device_math/kmer_summary.hip, built with the product's flags);
  2. whole reads, the restatement computed from what the same batch returned (borders, the aligned signal, the k-mer codes);
  3. the same integers through every path that aligns; accumulation, reset, and the switch off changing nothing;
  4. dynamont-resquiggle --kmer-summary, one process and two ranks: the same bytes.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kmer_summary_cases as ksc
from conftest import ROOT, model_for
from dynamont_amd import Aligner, _native, synth
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel, write_kmer_summary

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

NAMES = ("n_segments", "n_samples", "q1_lo", "q1_hi", "q2_lo", "q2_hi")


def assert_equal(got_cols, got_totals, want, what=""):
    """the six uint64 arrays and the totals against a restated accumulator, with the first k-mers that differ"""
    want_cols, want_totals = ksc.limbs(want)
    for name, g, w in zip(NAMES, got_cols, want_cols):
        bad = np.flatnonzero(np.asarray(g, dtype=np.uint64) != w)
        assert bad.size == 0, "%s %s: k-mers %s device %s restatement %s" % (what, name, bad[:5], [hex(int(g[c])) for c in bad[:5]],
                                                                            [hex(int(w[c])) for c in bad[:5]])
    assert [int(v) for v in got_totals] == [int(v) for v in want_totals], (what, list(got_totals), list(want_totals))


def assert_summary(s, want, what=""):
    assert_equal(s["limbs"], [s["totals"][k] for k in ksc.TOTALS], want, what)
    assert [int(v) for v in s["Q1"]] == want["Q1"] and [int(v) for v in s["Q2"]] == want["Q2"], what


# ---- 1. the device harness ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("ksum") / "libksum.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/kmer_summary.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.ks_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def batch():
    return ksc.build_batch()


def run_harness(lib, b, lo=0, hi=None, runs=1):
    acc = np.full(b.num_kmers * 6 + 4, 0xdeadbeef, dtype=np.uint64)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.ks_run(C.c_int(len(b.read)), p(b.sig_off), p(b.par_off), p(b.seg_off), p(b.T), p(b.N), p(b.read), C.c_int(len(b.status)),
                   p(b.status), C.c_uint64(len(b.sig)), p(b.sig), C.c_uint64(len(b.segrow)), p(b.segrow), C.c_uint64(len(b.kmers)),
                   p(b.kmers), C.c_uint32(b.num_kmers), C.c_uint32(lo), C.c_uint32(len(b.reads) if hi is None else hi), C.c_int(runs),
                   p(acc), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    cells = acc[:b.num_kmers * 6].reshape(b.num_kmers, 6)
    return [cells[:, f].copy() for f in range(6)], acc[b.num_kmers * 6:].copy()


def test_device_harness_every_integer(harness, batch):
    """segments of 1 .. 20 001 samples, 5 000 segments from many blocks on one k-mer, q1 = +-2^70 on one k-mer, q2 at 2^100,
    S2 = 2^64 and the double below, a failed read between ok reads, -0.0 and denormals (tests/test_kmer_summary_host.py shows
    that a dropped carry, a truncated q and a missing sign extension each change these sums). Twice: the same bits."""
    want = ksc.reference(batch)
    first = run_harness(harness, batch)
    assert_equal(*first, want, "run 1")
    second = run_harness(harness, batch)
    assert all(np.array_equal(a, b) for a, b in zip(first[0], second[0])) and np.array_equal(first[1], second[1])


def test_device_harness_read_range_and_accumulation(harness, batch):
    """the reads [2, 9) only (a merged launch whose members did not all ask), and two launches into one accumulator"""
    assert_equal(*run_harness(harness, batch, 2, 9), ksc.reference(batch, 2, 9), "reads 2..8")
    once = ksc.reference(batch)
    assert_equal(*run_harness(harness, batch, runs=2), ksc.summed(once, once), "two launches")
    cols, totals = run_harness(harness, batch, 5, 5)
    assert not any(c.any() for c in cols) and not totals.any()


# ---- 2. whole reads ------------------------------------------------------------------------------------------------------------
def restate(al, res, signals, seqs, acc=None, per_read=None):
    """the definition over what the batch returned: every ok read's borders, the signal it aligned, its k-mer codes"""
    acc = ksc.empty(al.num_kmers) if acc is None else acc
    status, _, codes = al.validate([len(s) for s in signals], seqs)
    for i in range(res.n):
        if res.status[i] != 0:
            continue
        assert status[i] == 0 and int(res.n_segments[i]) == len(codes[i])   # one output row per k-mer
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        ksc.add_aligned_read(acc, codes[i], signals[i], res.signal_positions[a:b])
        if per_read is not None:
            per_read.append(ksc.add_aligned_read(ksc.empty(al.num_kmers), codes[i], signals[i], res.signal_positions[a:b]))
    return acc


def run_batch(al, sig, seq):
    """a synchronous batch, its results and the device-resident signal of every read (Batch.signals())"""
    with al.batch(sig, seq) as b:
        b.align(True)
        res = b.fetch()
        x = b.signals()
    off = np.concatenate([[0], np.cumsum([len(v) for v in sig])]).astype(np.int64)
    return res, [x[int(off[i]):int(off[i + 1])] for i in range(len(sig))]


def polya_reads(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    return synth.make_reads(6101, 48, "rna002", mean, sd, (150, 300), polya=(20, 150))


def test_rna002_5mers_every_kmer_collides(models):
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn5"], "rna002", device=0)
    with pytest.raises(ValueError, match="never called"):
        al.kmer_summary()
    al.set_kmer_summary(True)
    res, xs = run_batch(al, sig, seq)
    assert (res.status == 0).all()
    want = restate(al, res, xs, seq)
    s = al.kmer_summary()
    assert_summary(s, want)
    assert s["totals"]["reads_ok"] == 48 and s["totals"]["segments"] == int(res.n_segments.sum()) > 8000
    assert s["totals"]["samples"] == sum(len(v) for v in sig) and s["totals"]["skipped_segments"] == 0
    assert s["n_segments"][0] > 48 * 20 and (s["n_segments"] > 1).sum() > 900      # AAAAA: the polyA rows; 1 024 codes collide
    al.close()


def test_synthetic_9mers_and_a_batch_aligned_twice_counts_twice(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6102, 24, "rna004", mean, sd, (100, 250))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_kmer_summary(True)
    with al.batch(sig, seq) as b:
        b.align(True)
        res = b.fetch()
        want = restate(al, res, sig, seq)
        assert_summary(al.kmer_summary(), want, "once")
        b.align(False)                       # a Z-only job adds nothing
        assert_summary(al.kmer_summary(), want, "after a Z-only job")
        al.set_kmer_summary(False)
        b.align(True)                        # the switch at submission decides
        assert_summary(al.kmer_summary(), want, "switch off")
        al.set_kmer_summary(True)
        b.align(True)
        assert_summary(al.kmer_summary(), ksc.summed(want, want), "twice")
    al.reset_kmer_summary()
    assert_summary(al.kmer_summary(), ksc.empty(al.num_kmers), "reset")
    al.close()


def test_stalled_pore_failed_reads_and_a_wide_band_read(models):
    """a ~20 000-sample segment (k_ksum_long beyond 256 chunks), a read that fails validation and one the Z check refuses
    inside the batch; then a DNA read of 480 bases at band 600 (the generic wide-band kernel)"""
    from test_gpu_event_stats import _fixed_dwell_read
    _, mean, sd = synth.read_model_file(models["syn9"])
    mean_c, sd_c = synth.code_order_table(mean, sd, 9, True)
    rng = np.random.default_rng(61)
    dw = np.maximum(2, rng.poisson(10, size=160))
    dw[60], dw[100], dw[120] = 20000, 257, 700
    stalled = _fixed_dwell_read(rng, mean_c, sd_c, 9, dw)
    reads = synth.make_reads(6103, 6, "rna004", mean, sd, (100, 200)) + [stalled]
    reads[1] = synth.SynthRead(reads[1].signal, reads[1].sequence[:40] + "N" + reads[1].sequence[41:])   # fails validation
    reads[3] = synth.SynthRead(np.full(len(reads[3].signal), np.inf), reads[3].sequence)                 # refused by the Z check
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_kmer_summary(True)
    res, xs = run_batch(al, sig, seq)
    assert res.status[1] != 0 and res.status[3] != 0 and (np.delete(res.status, [1, 3]) == 0).all()
    assert res.error(3) == "Alignment failed: alignment scores do not match"
    want = restate(al, res, xs, seq)
    s = al.kmer_summary()
    assert_summary(s, want)
    assert s["totals"]["reads_ok"] == 5 and s["totals"]["skipped_segments"] == 0
    L = np.diff(np.append(res.read(6)["signal_positions"].astype(np.int64), len(sig[6])))
    assert L.max() > 16384 and (L > 256).sum() >= 2
    al.close()
    pore = "dna_r10_400bps"
    wide = synth.make_reads(6104, 1, pore, mean, sd, 480) + synth.make_reads(6105, 2, pore, mean, sd, (100, 200))
    sig, seq = [r.signal for r in wide], [r.sequence for r in wide]
    al = Aligner(models["syn9"], pore, band=600, device=0)
    al.set_kmer_summary(True)
    res, xs = run_batch(al, sig, seq)
    assert (res.status == 0).all()
    assert_summary(al.kmer_summary(), restate(al, res, xs, seq), "band 600")
    al.close()


def test_rescaling_job_counts_once_with_its_last_signal(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6106, 12, "rna004", mean, sd, (100, 200))
    sig, seq = [np.ascontiguousarray(1.2 * r.signal + 0.3) for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_rescale(1)
    al.set_kmer_summary(True)
    res, xs = run_batch(al, sig, seq)
    assert (res.status == 0).all() and (res.rescale_iters == 1).sum() >= 10
    assert sum(not np.array_equal(x, s0) for x, s0 in zip(xs, sig)) >= 10          # the signal the last pass aligned is not the input
    s = al.kmer_summary()
    assert_summary(s, restate(al, res, xs, seq))
    assert s["totals"]["reads_ok"] == 12                                            # two passes, counted once
    al.close()


# ---- 3. the same integers through every path ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_tickets(models):
    """the 48 polyA reads repeated to 512 reads, twice (the second ticket starts at read 7): the tickets, and the summary of each
    restated from ONE synchronous batch of the 48 reads (a read's result does not depend on its neighbours)"""
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn5"], "rna002", device=0)
    res = al.align_batch(sig, seq, True)
    per_read = []
    restate(al, res, sig, seq, per_read=per_read)
    al.close()
    tickets, wants = [], []
    for start in (0, 7):
        idx = [(start + j) % 48 for j in range(512)]
        tickets.append(([reads[i] for i in idx], synth.pack_reads([reads[i] for i in idx])))
        w = ksc.empty(1024)
        for i in idx:
            w = ksc.summed(w, per_read[i])
        wants.append(w)
    return tickets, wants, res


def _async(al, tickets, order=(0, 1)):
    ts = [al.align_async(*tickets[j][1], True) for j in order]
    out = []
    for t in ts:
        res = t.wait()
        out.append((res, t.timing()))
        t.close()
    return out


def test_resident_session(models, two_tickets):
    tickets, wants, base = two_tickets
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_kmer_summary(True)
    done = _async(al, tickets)
    assert all(tm["launches"] == 0 for _, tm in done)                # both published into the resident session
    assert_summary(al.kmer_summary(), ksc.summed(*wants))
    m = int(base.seg_offsets[-1])
    assert np.array_equal(done[0][0].signal_positions[:m], base.signal_positions[:m])
    st = al.session_stats()
    assert st["tickets"] >= 2 and st["aborted"] == 0                 # the summary threw no ticket out of the session
    al.close()


def test_one_launch_per_ticket_and_synchronous_batches(models, two_tickets):
    tickets, wants, _ = two_tickets
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_session_mode(False)
    al.set_kmer_summary(True)
    singles = []
    for reads, _ in tickets:                                         # one synchronous align_batch per ticket: the singles
        al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True)
        singles.append(al.kmer_summary())
        al.reset_kmer_summary()
    for s, w in zip(singles, wants):
        assert_summary(s, w, "single")
    done = _async(al, tickets)                                       # asynchronous, no session: accumulation over the two
    assert all(tm["launches"] == 1 for _, tm in done)
    both = al.kmer_summary()
    assert_summary(both, ksc.summed(*wants), "two tickets")
    # ... equals the sum of the two singles, as integers
    assert [int(a) + int(b) for a, b in zip(singles[0]["Q1"], singles[1]["Q1"])] == [int(v) for v in both["Q1"]]
    assert [int(a) + int(b) for a, b in zip(singles[0]["Q2"], singles[1]["Q2"])] == [int(v) for v in both["Q2"]]
    assert np.array_equal(singles[0]["n_samples"] + singles[1]["n_samples"], both["n_samples"])
    al.reset_kmer_summary()
    z = al.kmer_summary()
    assert not any(c.any() for c in z["limbs"]) and not any(z["totals"].values())
    al.close()


def test_merged_tickets_and_a_switch_that_changes_in_flight(models, two_tickets):
    tickets, wants, _ = two_tickets
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_session_mode(False)
    al.set_kmer_summary(True)
    merged = False
    for attempt in range(3):   # (whether tickets meet in the queue is a matter of timing)
        al.reset_kmer_summary()
        done = _async(al, tickets, order=(0, 1, 0, 1))               # depth 4
        w = ksc.summed(*wants)
        assert_summary(al.kmer_summary(), ksc.summed(w, w), "depth 4, attempt %d" % attempt)
        merged |= any(tm["launch_share"] < 1.0 for _, tm in done)
        if merged:
            break
    assert merged
    # the switch is snapshot per ticket: tickets submitted while it is off add nothing, merged with others or not
    al.reset_kmer_summary()
    ts = []
    for j in (0, 1, 0, 1):
        al.set_kmer_summary(j == 0)
        ts.append(al.align_async(*tickets[j][1], True))
    for t in ts:
        t.wait()
        t.close()
    assert_summary(al.kmer_summary(), ksc.summed(wants[0], wants[0]), "tickets 0 and 2 only")
    al.close()


def test_page_starved_session(models, two_tickets, monkeypatch):
    monkeypatch.setenv("DYN_FORCE_LAYOUT", "separate")
    tickets, wants, _ = two_tickets
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_mem_budget(1 << 30)
    al.set_kmer_summary(True)
    done = _async(al, tickets)
    longest = max(len(r.signal) for r in tickets[0][0])
    for _, tm in done:
        print("paged session: pool_pages %d, page_rows %d, n_waves %d, longest read %d samples" % (
            tm["pool_pages"], tm["page_rows"], tm["n_waves"], longest))
        assert tm["launches"] == 0
        assert tm["pool_pages"] < tm["n_waves"] * -(-(longest + 1) // tm["page_rows"])   # no arena per wave: pages are shared
    assert_summary(al.kmer_summary(), ksc.summed(*wants))
    al.close()


def test_switch_off_changes_nothing(models, two_tickets):
    tickets, _, _ = two_tickets
    reads = tickets[0][0][:96]
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn5"], "rna002", device=0)
    off = al.align_batch(sig, seq, True)
    with pytest.raises(ValueError, match="never called"):
        al.kmer_summary()
    with pytest.raises(ValueError, match="never called"):
        al.reset_kmer_summary()
    al.set_kmer_summary(True)
    on = al.align_batch(sig, seq, True)
    al.set_kmer_summary(False)
    again = al.align_batch(sig, seq, True)
    m = int(off.seg_offsets[-1])
    for other in (on, again):
        for col in ("Z", "status", "n_segments", "seg_offsets"):
            assert np.asarray(getattr(off, col)).tobytes() == np.asarray(getattr(other, col)).tobytes(), col
        for col in ("signal_positions", "sequence_positions", "probabilities", "states"):
            assert getattr(off, col)[:m].tobytes() == getattr(other, col)[:m].tobytes(), col
    assert al.kmer_summary()["totals"]["reads_ok"] == 96             # the job submitted while it was on, and only that one
    al.close()


# ---- 4. the CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_writes_the_apis_integers_for_one_and_two_ranks(models, tmp_path):
    from test_gpu_multirank_cli import _torchrun
    pore = "rna002"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(6201, 11, pore, mean, sd, (60, 200))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "ks", reads, pore, seed=6, container="pod5", basecalls="bam")
    base = ["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "3"]
    seg.main(base + ["-o", str(tmp_path / "one.csv"), "--kmer-summary", str(tmp_path / "one.tsv")])
    # the API on the signals the CLI aligns (normalised, Hampel-filtered) and the sequences it hands the aligner
    sig, seq = [], []
    for x, s in expected:
        x = x.copy()
        hampel(x)
        sig.append(x)
        seq.append(s)
    al = Aligner(model, pore, device=0)
    al.set_kmer_summary(True)
    res = al.align_batch(sig, seq, True)
    assert (res.status == 0).all()
    s = al.kmer_summary()
    assert_summary(s, restate(al, res, sig, seq))
    write_kmer_summary(str(tmp_path / "api.tsv"), s, model, *al.model_table(), al.rna)
    al.close()
    one = open(tmp_path / "one.tsv", "rb").read()
    assert one == open(tmp_path / "api.tsv", "rb").read() and one.count(b"\n") == 1025
    assert sum(int(ln.split(b"\t")[3]) for ln in one.split(b"\n")[1:-1]) == s["totals"]["segments"]
    # the file is a model: the handle built from it aligns
    al2 = Aligner(str(tmp_path / "one.tsv"), pore, device=0)
    assert (al2.align_batch(sig[:2], seq[:2], True).status == 0).all()
    al2.close()
    _torchrun("dynamont_amd.segmentation.segment", base + ["-o", str(tmp_path / "two.csv"), "--kmer-summary", str(tmp_path / "two.tsv")], 29651)
    assert open(tmp_path / "two.tsv", "rb").read() == one
