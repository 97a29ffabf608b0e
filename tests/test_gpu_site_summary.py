"""GPU (-m gpu): the per-site level summary (Aligner.set_site_summary, site_summary.hip). All seven integers of every site and the
five totals must EQUAL the Python-int restatement of the definition (tests/site_summary_cases.py):
  1. the product's kernels on path arrays of the test's own (tests/device_math/site_summary.hip, built with the product's flags);
  2. whole reads through Aligner: the restatement applied to the borders the same job returned and the signal it aligned, the
     ids keyed by base j + k // 2; cross-checked against rint(level_mean * 2**40) of set_event_stats(True);
  3. the same integers through every path that aligns: merged tickets, raw tickets, a resident session, rescaling, the guide
     rescue; the switch off changing nothing; reset; the setter called with another size while a ticket is in flight.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess
from collections import Counter

import numpy as np
import pytest

import site_summary_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth
from dynamont_amd.sites import DYN_SITE_NONE, to_aligner_orientation

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

NAMES = ("n_rows", "n_samples", "dwell_sq", "m1_lo", "m1_hi", "m2_lo", "m2_hi")


def assert_equal(got_cols, got_totals, want, what=""):
    """the seven uint64 arrays and the totals against a restated table, with the first sites that differ"""
    want_cols, want_totals = ssc.limbs(want)
    for name, g, w in zip(NAMES, got_cols, want_cols):
        g = np.asarray(g, dtype=np.uint64)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s %s: sites %s device %s restatement %s" % (what, name, bad[:5], [hex(int(g[c])) for c in bad[:5]],
                                                                           [hex(int(w[c])) for c in bad[:5]])
    assert [int(v) for v in got_totals] == [int(v) for v in want_totals], (what, list(got_totals), list(want_totals))


def assert_summary(s, want, what=""):
    assert_equal(s["limbs"], [s["totals"][k] for k in ssc.TOTALS], want, what)
    assert [int(v) for v in s["M1"]] == want["M1"] and [int(v) for v in s["M2"]] == want["M2"], what


# ---- 1. the device harness ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("ssum") / "libssum.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/site_summary.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.ss_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def batch():
    return ssc.build_batch()


def run_harness(lib, b, lo=0, hi=None, runs=1, num_sites=None):
    ns = b.num_sites if num_sites is None else num_sites
    acc = np.full(ns * 7 + 5, 0xdeadbeef, dtype=np.uint64)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.ss_run(C.c_int(len(b.read)), p(b.sig_off), p(b.par_off), p(b.seg_off), p(b.T), p(b.N), p(b.read), C.c_int(len(b.status)),
                   p(b.status), C.c_uint64(len(b.sig)), p(b.sig), C.c_uint64(len(b.segrow)), p(b.segrow), C.c_uint64(len(b.sites)),
                   p(b.sites), C.c_uint32(ns), C.c_uint32(lo), C.c_uint32(len(b.reads) if hi is None else hi), C.c_int(runs),
                   p(acc), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    cells = acc[:ns * 7].reshape(ns, 7)
    return [cells[:, f].copy() for f in range(7)], acc[ns * 7:].copy()


def test_device_harness_every_integer(harness, batch):
    """rows of 1, 63, 64, 65, 256, 257, 16 384 and 16 392 samples; DYN_SITE_NONE, num_sites - 1 and num_sites in both kernels;
    600 rows of level +-2^22 on one site (tests/test_site_summary_host.py shows that a dropped carry, a missing sign extension,
    a truncated m1 and m = S1 * (1 / L) each change these sums); m * m = 2^64, NaN and infinite samples; a failed read.
    Twice: the same bits."""
    want = ssc.reference(batch)
    first = run_harness(harness, batch)
    assert_equal(*first, want, "run 1")
    t = want["totals"]
    assert t["rows_without_site"] >= 4 and t["rows_skipped"] >= 8 and t["reads_ok"] == len(batch.reads) - 1
    assert want["M1"][11] >> 64 != 0 and want["M1"][12] < 0 and want["n_rows"][11] == 600      # the carry reached the high limb
    second = run_harness(harness, batch)
    assert all(np.array_equal(a, b) for a, b in zip(first[0], second[0])) and np.array_equal(first[1], second[1])


def test_device_harness_read_range_one_site_and_accumulation(harness, batch):
    """the reads [2, 9) only (a merged launch whose members did not all ask), a table of ONE site, two launches into one table"""
    assert_equal(*run_harness(harness, batch, 2, 9), ssc.reference(batch, 2, 9), "reads 2..8")
    one = ssc.reference(batch, num_sites=1)
    assert one["n_rows"] == [1] and one["totals"]["rows_skipped"] > 600
    assert_equal(*run_harness(harness, batch, num_sites=1), one, "num_sites = 1")
    once = ssc.reference(batch)
    assert_equal(*run_harness(harness, batch, runs=2), ssc.summed(once, once), "two launches")
    cols, totals = run_harness(harness, batch, 5, 5)
    assert not any(c.any() for c in cols) and not totals.any()


# ---- 2. whole reads ------------------------------------------------------------------------------------------------------------
NUM_SITES = 3000


def make_ids(reads, seed, num_sites=NUM_SITES, span=None):
    """per-base ids of every read: a window of consecutive sites at a random start (reads overlap: span << total bases), runs of
    DYN_SITE_NONE inside, and a few bases whose id lies outside the table"""
    rng = np.random.default_rng(seed)
    span = span or num_sites // 3
    out = []
    for r in reads:
        n = len(r.sequence)
        ids = (int(rng.integers(0, span)) + np.arange(n, dtype=np.int64)).astype(np.uint32)
        for _ in range(1 + n // 60):
            a = int(rng.integers(0, n))
            ids[a:a + int(rng.integers(1, 9))] = DYN_SITE_NONE
        ids[int(rng.integers(0, n))] = num_sites + int(rng.integers(0, 5))
        out.append(ids)
    return out


def restate(al, res, signals, ids, num_sites=NUM_SITES, acc=None, per_read=None, idx=None):
    """the definition over what the job returned: every ok read's borders, the signal it aligned, its per-base ids"""
    acc = ssc.empty(num_sites) if acc is None else acc
    for i in range(res.n) if idx is None else idx:
        if res.status[i] != 0:
            if per_read is not None:
                per_read.append(None)
            continue
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        assert b - a == len(ids[i]) - al.kmer_size + 1                       # one output row per lattice column
        ssc.add_aligned_read(acc, ids[i], al.kmer_size, signals[i], res.signal_positions[a:b])
        if per_read is not None:
            per_read.append(ssc.add_aligned_read(ssc.empty(num_sites), ids[i], al.kmer_size, signals[i], res.signal_positions[a:b]))
    return acc


def run_batch(al, sig, seq, ids):
    """a synchronous batch with ids, its results and the device-resident signal of every read (Batch.signals())"""
    with al.batch(sig, seq, site_ids=np.concatenate(ids)) as b:
        b.align(True)
        res = b.fetch()
        x = b.signals()
    off = np.concatenate([[0], np.cumsum([len(v) for v in sig])]).astype(np.int64)
    return res, [x[int(off[i]):int(off[i + 1])] for i in range(len(sig))]


def test_align_batch_48_reads_and_the_event_means(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6301, 48, "dna_r10_400bps", mean, sd, (40, 400), dwell=13.0)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    assert min(len(s) for s in sig) >= 300 and max(len(s) for s in sig) <= 6000
    ids = make_ids(reads, 1)
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    with pytest.raises(ValueError, match="never called"):
        al.site_summary()
    al.set_site_summary(NUM_SITES)
    al.set_event_stats(True)
    res = al.align_batch(sig, seq, True, site_ids=np.concatenate(ids))
    assert (res.status == 0).all()
    want = restate(al, res, sig, ids)
    s = al.site_summary()
    assert_summary(s, want)
    t = s["totals"]
    assert t["reads_ok"] == 48 and 0 < t["rows_skipped"] <= 48                              # the ids outside the table
    assert t["rows_added"] + t["rows_without_site"] + t["rows_skipped"] == int(res.n_segments.sum())
    assert t["rows_without_site"] > 48 and (s["n_rows"] > 1).sum() > 500                    # NONE runs; overlapping reads
    # a row keyed by ids[j] instead of ids[j + k // 2] gives another table from the same job
    wrong = ssc.empty(NUM_SITES)
    for i in range(res.n):
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        ssc.add_aligned_read(wrong, ids[i], al.kmer_size, sig[i], res.signal_positions[a:b], shift=0)
    assert wrong["n_rows"] != want["n_rows"]
    # cross-check: rint(level_mean * 2**40) of the job's own event columns, summed per site, is M1 exactly
    m1 = [0] * NUM_SITES
    h = al.kmer_size // 2
    for i in range(res.n):
        a, n = int(res.seg_offsets[i]), int(res.n_segments[i])
        for j in range(n):
            sid = int(ids[i][j + h])
            if sid < NUM_SITES:
                m1[sid] += ssc.rint_scaled(res.level_mean[a + j])
    assert m1 == [int(v) for v in s["M1"]]
    # a window of the table, and a window outside it
    w = al.site_summary(100, 900)
    assert all(np.array_equal(c, f[100:900]) for c, f in zip(w["limbs"], s["limbs"])) and w["totals"] == s["totals"]
    with pytest.raises(ValueError, match="not a range"):
        al.site_summary(0, NUM_SITES + 1)
    # a count that differs from the batch's bases: refused, and consumed -- the next batch has no ids and adds nothing
    with pytest.raises(ValueError, match="staged"):
        al.align_batch(sig, seq, True, site_ids=np.concatenate(ids)[:-1])
    al.align_batch(sig, seq, True)
    assert_summary(al.site_summary(), want, "after a refused staging and a job without ids")
    al.reset_site_summary()
    assert_summary(al.site_summary(), ssc.empty(NUM_SITES), "reset")
    al.close()


def polya_reads(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    return synth.make_reads(6101, 48, "rna002", mean, sd, (150, 300), polya=(20, 150))


def test_rna_handle_with_the_pad_and_a_read_that_fails_validation(models):
    """ids made the way a caller makes them for RNA (dynamont_amd.sites): stored order reversed, DYN_SITE_NONE for the pad. One
    read fails validation in the middle of the batch: the per-row ids of the ok reads behind it are not shifted. A Z-only job and
    a train job consume their ids and add nothing."""
    reads = polya_reads(models)[:24]
    reads[11] = synth.SynthRead(reads[11].signal, reads[11].sequence[:40] + "N" + reads[11].sequence[41:])
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    rng = np.random.default_rng(5)
    ids = []
    for s in seq:
        stored = (int(rng.integers(0, 800)) + np.arange(len(s) - 9)).astype(np.uint32)   # the basecall without the pad, 5' -> 3'
        ids.append(to_aligner_orientation(stored, True, 9))
        assert len(ids[-1]) == len(s) and (ids[-1][:9] == DYN_SITE_NONE).all() and ids[-1][9] == stored[-1]
    al = Aligner(models["syn5"], "rna002", device=0)
    assert al.rna
    al.set_site_summary(1200)
    res, xs = run_batch(al, sig, seq, ids)
    assert res.status[11] != 0 and (np.delete(res.status, 11) == 0).all()
    want = restate(al, res, xs, ids, 1200)
    s = al.site_summary()
    assert_summary(s, want)
    assert s["totals"]["reads_ok"] == 23 and s["totals"]["rows_without_site"] == 23 * (9 - al.kmer_size // 2)
    flat = np.concatenate(ids)
    with al.batch(sig, seq, site_ids=flat) as b:
        b.align(False)
    with al.batch(sig, seq, site_ids=flat) as b:
        b.train()
    assert_summary(al.site_summary(), want, "after a Z-only and a train job")
    al.close()


def test_rescaling_job_counts_once_with_its_last_signal(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6106, 12, "rna004", mean, sd, (100, 200))
    sig, seq = [np.ascontiguousarray(1.2 * r.signal + 0.3) for r in reads], [r.sequence for r in reads]
    ids = make_ids(reads, 2)
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_rescale(1)
    al.set_site_summary(NUM_SITES)
    res, xs = run_batch(al, sig, seq, ids)
    assert (res.status == 0).all() and (res.rescale_iters == 1).sum() >= 10
    assert sum(not np.array_equal(x, s0) for x, s0 in zip(xs, sig)) >= 10          # the signal the last pass aligned is not the input
    s = al.site_summary()
    assert_summary(s, restate(al, res, xs, ids))
    assert s["totals"]["reads_ok"] == 12                                            # two passes, counted once
    al.close()


def test_guide_rescue_counts_once_behind_the_rescue(models):
    import guide_rescue_cases as rc
    import guided_band_cases as gc
    _, mean, sd = synth.read_model_file(models["syn5"])
    reads, _, _ = rc.mixed(gc.build_reads(mean, sd))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    ids = make_ids(reads, 3)
    al = Aligner(models["syn5"], gc.PORE, band=rc.BAND, device=0)
    al.set_site_summary(NUM_SITES)
    al.set_guide_rescue(1, 16, 8)
    res, xs = run_batch(al, sig, seq, ids)
    assert (res.rescue == 1).sum() >= 3
    ok = int((res.status == 0).sum())
    s = al.site_summary()
    assert_summary(s, restate(al, res, xs, ids))                                    # the borders the rescue left
    assert s["totals"]["reads_ok"] == ok
    al.set_guide_rescue(0, 0)
    al.reset_site_summary()
    plain, xs = run_batch(al, sig, seq, ids)
    m = int(res.seg_offsets[-1])
    assert not np.array_equal(plain.signal_positions[:m], res.signal_positions[:m])  # ... which are not the plain ones
    assert_summary(al.site_summary(), restate(al, plain, xs, ids), "plain")
    al.close()


# ---- 3. tickets ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tickets(models):
    """the 48 polyA reads repeated to 512 reads, four times (ticket j starts at read 7 j), ids per ticket; and every read's own
    table restated from ONE synchronous batch of the 48 (a read's result does not depend on its neighbours)"""
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn5"], "rna002", device=0)
    res = al.align_batch(sig, seq, True)
    assert (res.status == 0).all()
    out = []
    for j in range(4):
        ids48 = make_ids(reads, 10 + j)
        per_read = []
        restate(al, res, sig, ids48, per_read=per_read)
        idx = [(7 * j + i) % 48 for i in range(512)]
        want = ssc.empty(NUM_SITES)
        for i, mult in Counter(idx).items():
            scaled = {c: [v * mult for v in per_read[i][c]] for c in ssc.COLS}
            scaled["totals"] = {k: v * mult for k, v in per_read[i]["totals"].items()}
            want = ssc.summed(want, scaled)
        out.append((synth.pack_reads([reads[i] for i in idx]), np.concatenate([ids48[i] for i in idx]), want))
    al.close()
    return out, res


def submit(al, tk, with_ids=True):
    packed, ids, _ = tk
    return al.align_async(*packed, True, site_ids=ids if with_ids else None)


def test_four_tickets_that_merge(models, tickets):
    """four tickets back to back, no session: two with ids, one without, one submitted with the switch off. They are queued
    behind a ticket that adds nothing (the switch on, no ids) and keeps the GPU busy, so that they wait together and share
    launches of two (Pipeline::merge: the members' ids concatenated, DYN_SITE_NONE for the member without, the read ranges of
    those that asked and staged). A ticket with ids can only be paired with a neighbour that contributes nothing, so a shared
    launch of ticket 0 or 2 is a mixed one. Whether tickets meet is still a matter of timing: three attempts, as the k-mer
    summary's counterpart has them, and the meeting is asserted."""
    tks, _ = tickets
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_session_mode(False)
    al.set_auto_guide(0)
    al.set_site_summary(NUM_SITES)
    want = ssc.summed(tks[0][2], tks[2][2])
    merged = False
    for attempt in range(3):
        al.reset_site_summary()
        ahead = submit(al, tks[3], with_ids=False)                   # on the GPU while the four below queue up
        ts = [submit(al, tks[0]), submit(al, tks[1], with_ids=False), submit(al, tks[2])]
        al.set_site_summary(0)
        ts.append(submit(al, tks[3]))                                # staged, but the switch is off at its submission
        al.set_site_summary(NUM_SITES)
        tms = []
        for t in [ahead] + ts:
            t.wait()
            tms.append(t.timing())
            t.close()
        assert_summary(al.site_summary(), want, "attempt %d" % attempt)
        print("attempt %d: launch shares" % attempt, [round(tm["launch_share"], 3) for tm in tms])
        merged |= tms[1]["launch_share"] < 1.0 or tms[3]["launch_share"] < 1.0   # ticket 0 or ticket 2: one with ids
        if merged:
            break
    assert merged
    al.close()


def test_resident_session_equals_one_launch_per_batch(models):
    """one ticket of 600 reads of about 300 samples opens a resident session; the same reads through one launch per batch
    (DYN_NO_SESSION through set_session_mode) give the same bits"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6302, 600, "rna004", mean, sd, (28, 36))
    ids = make_ids(reads, 4, span=300)
    packed, flat = synth.pack_reads(reads), np.concatenate(ids)
    tables = []
    for session in (True, False):
        al = Aligner(models["syn9"], "rna004", device=0)
        al.set_session_mode(session)
        al.set_site_summary(NUM_SITES)
        with al.align_async(*packed, True, site_ids=flat) as t:
            res = t.wait()
            tm = t.timing()
            x = t.signals(len(packed[0]))
        assert tm["launches"] == (0 if session else 1)
        if session:
            st = al.session_stats()
            assert st["tickets"] >= 1 and st["aborted"] == 0
            off = packed[1].astype(np.int64)
            want = restate(al, res, [x[off[i]:off[i + 1]] for i in range(600)], ids)
        tables.append(al.site_summary())
        al.close()
    assert_summary(tables[0], want, "session")
    assert_summary(tables[1], want, "one launch")
    assert all(np.array_equal(a, b) for a, b in zip(tables[0]["limbs"], tables[1]["limbs"])) and tables[0]["totals"] == tables[1]["totals"]


def test_raw_ticket_int16_with_calibration(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6303, 40, "rna004", mean, sd, (60, 160))
    rng = np.random.default_rng(6)
    n = len(reads)
    shift, scale = rng.uniform(80, 120, n), rng.uniform(10, 20, n)
    cal_off, cal_scale = rng.uniform(-5, 5, n).astype(np.float32), rng.uniform(0.1, 0.2, n).astype(np.float32)
    raw = [np.round((r.signal * sc + sh) / cs - co).astype(np.int16) for r, sh, sc, co, cs in zip(reads, shift, scale, cal_off, cal_scale)]
    seq = [r.sequence for r in reads]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in raw])
    seq_off = np.zeros(n + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seq])
    ids = make_ids(reads, 7)
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_site_summary(NUM_SITES)
    with al.align_raw_async(np.concatenate(raw), off, shift, scale, "".join(seq).encode(), seq_off, calibration=(cal_off, cal_scale),
                            site_ids=np.concatenate(ids)) as t:
        res = t.wait()
        x = t.signals(int(off[-1]))
    assert (res.status == 0).sum() >= 36
    o = off.astype(np.int64)
    s = al.site_summary()
    assert_summary(s, restate(al, res, [x[o[i]:o[i + 1]] for i in range(n)], ids))
    assert s["totals"]["reads_ok"] == int((res.status == 0).sum())
    al.close()


def test_switch_off_changes_nothing(models, tickets):
    tks, _ = tickets
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    flat = np.concatenate(make_ids(reads, 8))
    al = Aligner(models["syn5"], "rna002", device=0)
    off = al.align_batch(sig, seq, True)
    staged = al.align_batch(sig, seq, True, site_ids=flat)           # the switch is off: consumed, ignored
    with pytest.raises(ValueError, match="never called"):
        al.site_summary()
    with pytest.raises(ValueError, match="never called"):
        al.reset_site_summary()
    al.set_site_summary(NUM_SITES)
    on = al.align_batch(sig, seq, True, site_ids=flat)
    m = int(off.seg_offsets[-1])
    for other in (staged, on):
        for col in ("Z", "status", "n_segments", "seg_offsets"):
            assert np.asarray(getattr(off, col)).tobytes() == np.asarray(getattr(other, col)).tobytes(), col
        for col in ("signal_positions", "sequence_positions", "probabilities", "states"):
            assert getattr(off, col)[:m].tobytes() == getattr(other, col)[:m].tobytes(), col
    assert al.site_summary()["totals"]["reads_ok"] == 48             # the job submitted while it was on, and only that one
    al.close()


def test_setter_with_another_size_while_a_ticket_is_in_flight(models, tickets):
    """the ticket holds the table it was submitted under: the setter waits for it, then starts a new, zeroed table"""
    tks, _ = tickets
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_site_summary(NUM_SITES)
    t = submit(al, tks[0])
    al.set_site_summary(NUM_SITES // 2)                              # returns once the ticket is done
    s = al.site_summary()
    assert len(s["n_rows"]) == NUM_SITES // 2 and not any(c.any() for c in s["limbs"]) and not any(s["totals"].values())
    res = t.wait()
    assert (res.status == 0).all()
    t.close()
    with submit(al, tks[1]) as t2:
        t2.wait()
    half = ssc.empty(NUM_SITES // 2)                                  # the same rows against a table half the size
    full = tks[1][2]
    moved = sum(full["n_rows"][NUM_SITES // 2:])
    for c in ssc.COLS:
        half[c] = full[c][:NUM_SITES // 2]
    half["totals"] = dict(full["totals"], rows_added=full["totals"]["rows_added"] - moved,
                          samples_added=full["totals"]["samples_added"] - sum(full["n_samples"][NUM_SITES // 2:]),
                          rows_skipped=full["totals"]["rows_skipped"] + moved)
    assert_summary(al.site_summary(), half, "the new table")
    al.close()
