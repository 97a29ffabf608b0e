"""GPU (-m gpu): the per-site histograms and quantiles (Aligner.set_site_histogram, site_histogram, site_quantiles). Every counter
and every output integer must EQUAL the restatement of the definition (tests/site_histogram_cases.py):
  1. the product's filling kernels on path arrays of the test's own (tests/device_math/site_histogram.hip, built with the
     product's flags): the site summary's batch and the edge, edge-neighbour and dwell rows behind it; the table unchanged;
  2. the product's quantile kernel on histograms the test uploads, for 4, 34, 66 and 256 counters per site;
  3. whole reads through Aligner: the restatement over the borders the job returned and the signal it aligned, level_mean of the
     job's own event columns binned in NumPy, the quantiles, and the interpolated median against the exact k-th smallest mean;
  4. the same bytes through a resident session and one launch per batch; rescaling; jobs that add nothing; reset; the setters
     while a ticket is in flight; the switch off changing nothing.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import site_histogram_cases as shc
import site_summary_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth
from test_gpu_site_summary import assert_equal, make_ids, polya_reads, restate, run_batch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

NUM_SITES = 3000
SPEC = (32, -4.0, 4.0)


# ---- 1. the device harness: filling ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("shist") / "libshist.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/site_histogram.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.sh_run.restype = C.c_int
    lib.sq_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def batch():
    return shc.build_batch()


@pytest.fixture(scope="module")
def table_want(batch):
    return {(lo, hi): ssc.reference(batch, lo, hi) for lo, hi in ((0, None), (2, 9))}


@pytest.fixture(scope="module")
def hist_want(batch):
    out = {(spec, 0, None): shc.flat(shc.reference(batch, *spec)) for spec in (shc.EXACT, shc.ROUNDED)}
    out[(shc.EXACT, 2, 9)] = shc.flat(shc.reference(batch, *shc.EXACT, read_lo=2, read_hi=9))
    return out


def run_fill(lib, b, spec, lo=0, hi=None, runs=1, hist_on=True, poison=0):
    bins, h_lo, h_hi = spec
    ns = b.num_sites
    acc = np.full(ns * 7 + 5, 0xdeadbeef, dtype=np.uint64)
    hist = np.full(ns * (bins + 18), poison, dtype=np.uint32)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.sh_run(C.c_int(len(b.read)), p(b.sig_off), p(b.par_off), p(b.seg_off), p(b.T), p(b.N), p(b.read), C.c_int(len(b.status)),
                   p(b.status), C.c_uint64(len(b.sig)), p(b.sig), C.c_uint64(len(b.segrow)), p(b.segrow), C.c_uint64(len(b.sites)),
                   p(b.sites), C.c_uint32(ns), C.c_uint32(lo), C.c_uint32(len(b.reads) if hi is None else hi), C.c_int(runs),
                   C.c_int(bins), C.c_double(h_lo), C.c_double(h_hi), C.c_int(1 if hist_on else 0), p(acc), p(hist), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    cells = acc[:ns * 7].reshape(ns, 7)
    return ([cells[:, f].copy() for f in range(7)], acc[ns * 7:].copy()), hist


def assert_counters(got, want, bins, what=""):
    got, want = np.asarray(got, dtype=np.uint32).reshape(-1, bins + 18), np.asarray(want, dtype=np.uint32).reshape(-1, bins + 18)
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: (site, counter) %s device %s restatement %s" % (what, bad[:6].tolist(), [int(got[s, c]) for s, c in bad[:6]],
                                                                               [int(want[s, c]) for s, c in bad[:6]])


@pytest.mark.parametrize("spec", [shc.EXACT, shc.ROUNDED], ids=["32_exact_width", "30_rounded_width"])
def test_device_harness_every_counter(harness, batch, table_want, hist_want, spec):
    """rows of 1 .. 40 000 samples through both kernels; samples on every edge of (32, -4, 4) and the doubles below them; the 527
    doubles within 8 ulp of the edges of (30, -3.3, 4.1); a failed read, skipped and site-less rows (no counter). The table's
    seven integers and five totals are what they are without the histograms. Twice: the same bits."""
    table, hist = run_fill(harness, batch, spec)
    assert_counters(hist, hist_want[(spec, 0, None)], spec[0], "run 1")
    assert_equal(*table, table_want[(0, None)], "the table beside the histograms")
    lv = hist.reshape(-1, spec[0] + 18)
    assert (lv[:, :spec[0] + 2].sum(axis=1) == table[0][0]).all() and (lv[:, spec[0] + 2:].sum(axis=1) == table[0][0]).all()   # n_rows
    table2, hist2 = run_fill(harness, batch, spec)
    assert np.array_equal(hist, hist2) and all(np.array_equal(a, b) for a, b in zip(table[0], table2[0]))


def test_device_harness_off_two_launches_and_a_read_range(harness, batch, table_want, hist_want):
    """hist = nullptr leaves a poisoned buffer untouched (and the table right); two launches into one table give twice the
    counts; the reads [2, 9) alone"""
    table, hist = run_fill(harness, batch, shc.EXACT, hist_on=False, poison=0xA5A5A5A5)
    assert (hist == 0xA5A5A5A5).all()
    assert_equal(*table, table_want[(0, None)], "histograms off")
    once = hist_want[(shc.EXACT, 0, None)]
    table, hist = run_fill(harness, batch, shc.EXACT, runs=2)
    assert_counters(hist, 2 * once, 32, "two launches")
    assert_equal(*table, ssc.summed(table_want[(0, None)], table_want[(0, None)]), "two launches")
    table, hist = run_fill(harness, batch, shc.EXACT, 2, 9)
    assert_counters(hist, hist_want[(shc.EXACT, 2, 9)], 32, "reads 2..8")
    assert_equal(*table, table_want[(2, 9)], "reads 2..8")
    assert hist.any() and not np.array_equal(hist, once)


# ---- 2. the device harness: quantiles ----------------------------------------------------------------------------------------------
def run_quantiles(lib, table, B, lo, hi, probs):
    cnt, P = hi - lo, len(probs)
    out = np.full((1 + 4 * P) * cnt, 0x5A5A5A5A, dtype=np.uint32)
    guard = np.array([0x13572468], dtype=np.uint32)
    q = np.array(probs, dtype=np.float64)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    t = np.ascontiguousarray(table, dtype=np.uint32)
    k = lib.sq_run(C.c_uint32(t.shape[0]), C.c_int(B - 2), p(t), C.c_uint32(lo), C.c_uint32(hi), p(q), C.c_int(P), p(out), p(guard), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert guard[0] == 0x13572468                                    # nothing written behind the output
    return out[:cnt], [out[cnt + f * cnt * P:cnt + (f + 1) * cnt * P].reshape(cnt, P) for f in range(4)]


@pytest.mark.parametrize("B", [4, 34, 66, 256])
def test_device_harness_quantiles(harness, B):
    """one group of lanes per site (B = 4), a group boundary (34), more than a wave at one counter per lane (66), the maximum
    (256). Empty sites, all mass under / over, a single count, a prefix sum that meets k at a bin's end, 2^31 in one counter;
    probabilities 0, 1e-12, 0.25, 0.5, 0.75, 1 and eight at once; windows [3, 3), [3, 4), [5, 72) and the whole table."""
    table = shc.quantile_tables()[B]
    for lo, hi, probs in ((0, 100, shc.PROBS), (0, 100, shc.PROBS8), (3, 3, shc.PROBS), (3, 4, shc.PROBS), (5, 72, shc.PROBS), (99, 100, (0.5,))):
        n, cols = run_quantiles(harness, table, B, lo, hi, probs)
        want_n, want = shc.quantile_arrays(table[lo:hi, :B].tolist(), probs)
        assert np.array_equal(n, want_n), (B, lo, hi)
        for name, g, w in zip(("rank", "bin", "below", "in_bin"), cols, want):
            bad = np.argwhere(g != w)
            assert bad.size == 0, (B, lo, hi, name, bad[:5].tolist(), [int(g[s, q]) for s, q in bad[:5]], [int(w[s, q]) for s, q in bad[:5]])


# ---- 3. whole reads ----------------------------------------------------------------------------------------------------------------
def restate_hist(al, res, signals, ids, spec, num_sites=NUM_SITES):
    h = shc.empty(num_sites, spec[0])
    for i in range(res.n):
        if res.status[i] != 0:
            continue
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        shc.add_aligned_read(h, ids[i], al.kmer_size, signals[i], res.signal_positions[a:b], *spec)
    return h


def assert_hist(got, want, what=""):
    lv, dw = np.array(want["level"], dtype=np.uint32), np.array(want["dwell"], dtype=np.uint32)
    assert got["level"].shape == lv.shape and got["dwell"].shape == dw.shape, what
    assert np.array_equal(got["level"], lv), (what, np.argwhere(got["level"] != lv)[:5].tolist())
    assert np.array_equal(got["dwell"], dw), (what, np.argwhere(got["dwell"] != dw)[:5].tolist())


def test_align_batch_48_reads_counters_quantiles_and_the_median(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6301, 48, "dna_r10_400bps", mean, sd, (40, 400), dwell=13.0)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    ids = make_ids(reads, 1)
    flat = np.concatenate(ids)
    plain = Aligner(models["syn9"], "dna_r10_400bps", device=0)      # the table of a handle that never heard of the histograms
    plain.set_site_summary(NUM_SITES)
    plain.align_batch(sig, seq, True, site_ids=flat)
    plain_table = plain.site_summary()
    plain.close()
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_summary\(a, num_sites > 0\) was never called on this handle"):
        al.set_site_histogram(*SPEC)
    al.set_site_summary(NUM_SITES)
    for call in (al.site_histogram, lambda: al.site_quantiles([0.5])):
        with pytest.raises(ValueError, match=r"dyn_aligner_set_site_histogram\(a, bins > 0, lo, hi\) was never called on this handle"):
            call()
    with pytest.raises(ValueError, match=r"bins 255 is not 0 \(off\) or 2 \.\. 254"):
        al.set_site_histogram(255, -4.0, 4.0)                        # the same texts as on a handle without a device
    with pytest.raises(ValueError, match="lo and hi must be finite with lo < hi"):
        al.set_site_histogram(32, 4.0, 4.0)
    al.set_site_histogram(*SPEC)
    al.set_event_stats(True)
    res = al.align_batch(sig, seq, True, site_ids=flat)
    assert (res.status == 0).all()
    h = al.site_histogram()
    assert h["bins"] == 32 and h["lo"] == -4.0 and h["hi"] == 4.0 and np.array_equal(h["edges"], -4.0 + 0.25 * np.arange(33))
    assert h["level"].dtype == np.uint32 and h["level"].shape == (NUM_SITES, 34) and h["dwell"].shape == (NUM_SITES, 16)
    assert_hist(h, restate_hist(al, res, sig, ids, SPEC))
    table = al.site_summary()
    assert np.array_equal(h["level"].sum(axis=1), table["n_rows"]) and np.array_equal(h["dwell"].sum(axis=1), table["n_rows"])
    assert all(np.array_equal(a, b) for a, b in zip(table["limbs"], plain_table["limbs"])) and table["totals"] == plain_table["totals"]
    assert (table["n_rows"] > 1).sum() > 500 and h["level"][:, 1:33].sum() > 0.9 * h["level"].sum()
    # level_mean of the job's own event columns, binned in NumPy with the definition's two operations
    lv = np.zeros((NUM_SITES, 34), dtype=np.uint32)
    per_site = [[] for _ in range(NUM_SITES)]
    half = al.kmer_size // 2
    inv_w = np.float64(32) / (np.float64(4.0) - np.float64(-4.0))
    for i in range(res.n):
        a, n = int(res.seg_offsets[i]), int(res.n_segments[i])
        sid = ids[i][half:half + n].astype(np.int64)
        m = np.asarray(res.level_mean[a:a + n], dtype=np.float64)
        u = (m - np.float64(-4.0)) * inv_w
        b = np.where(u < 0, 0, np.where(u >= 32, 33, 1 + np.minimum(u, 32).astype(np.int64)))
        keep = sid < NUM_SITES
        np.add.at(lv, (sid[keep], b[keep]), 1)
        for s, v in zip(sid[keep].tolist(), m[keep].tolist()):
            per_site[s].append(v)
    assert np.array_equal(lv, h["level"])
    # the quantiles, and a window of them
    q = al.site_quantiles([0.25, 0.5, 0.75])
    want_n, want = shc.quantile_arrays(h["level"].tolist(), (0.25, 0.5, 0.75))
    assert np.array_equal(q["n"], want_n) and np.array_equal(q["n"], table["n_rows"].astype(np.uint32))
    for name, w in zip(("rank", "bin", "below", "in_bin"), want):
        assert np.array_equal(q[name], w), name
    assert q["level"].shape == (NUM_SITES, 3) and np.isnan(q["level"][q["n"] == 0]).all() and (q["bin"][q["n"] == 0] == shc.NO_BIN).all()
    win = al.site_quantiles([0.5], 101, 168)
    assert np.array_equal(win["bin"][:, 0], q["bin"][101:168, 1]) and np.array_equal(win["n"], q["n"][101:168])
    hw = al.site_histogram(100, 900)
    assert np.array_equal(hw["level"], h["level"][100:900]) and np.array_equal(hw["dwell"], h["dwell"][100:900])
    assert al.site_quantiles([0.5], 7, 7)["n"].size == 0
    # the interpolated median against the exact k-th smallest event mean of the site: both lie in the same bin, an interval of
    # width w = 0.25 (the bin's edges as the two operations of the definition draw them), so they differ by less than w
    checked = 0
    for s in np.flatnonzero(q["n"]).tolist():
        b = int(q["bin"][s, 1])
        if 1 <= b <= 32:
            exact = sorted(per_site[s])[int(q["rank"][s, 1]) - 1]
            assert abs(q["level"][s, 1] - exact) < 0.25, (s, q["level"][s, 1], exact)
            checked += 1
    assert checked > 500
    # the window checks and refusals behave as the table's do
    for call in (lambda: al.site_histogram(0, NUM_SITES + 1), lambda: al.site_quantiles([0.5], 0, NUM_SITES + 1),
                 lambda: al.site_quantiles([0.5], 9, 8)):
        with pytest.raises(ValueError, match=r"is not a range of the table's 3000 sites"):
            call()
    al.close()


# ---- 4. paths ------------------------------------------------------------------------------------------------------------------------
def test_resident_session_equals_one_launch_per_batch(models):
    """the site summary's own 600-read case: one ticket in a resident session against one launch per batch, identical bytes"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6302, 600, "rna004", mean, sd, (28, 36))
    ids = make_ids(reads, 4, span=300)
    packed, flat = synth.pack_reads(reads), np.concatenate(ids)
    got = []
    for session in (True, False):
        al = Aligner(models["syn9"], "rna004", device=0)
        al.set_session_mode(session)
        al.set_site_summary(NUM_SITES)
        al.set_site_histogram(*SPEC)
        with al.align_async(*packed, True, site_ids=flat) as t:
            res = t.wait()
            tm = t.timing()
            x = t.signals(len(packed[0]))
        assert tm["launches"] == (0 if session else 1)
        if session:
            off = packed[1].astype(np.int64)
            want = restate_hist(al, res, [x[off[i]:off[i + 1]] for i in range(600)], ids, SPEC)
        got.append((al.site_histogram(), al.site_summary()))
        al.close()
    assert_hist(got[0][0], want, "session")
    assert got[0][0]["level"].tobytes() == got[1][0]["level"].tobytes() and got[0][0]["dwell"].tobytes() == got[1][0]["dwell"].tobytes()
    assert np.array_equal(got[0][0]["level"].sum(axis=1), got[0][1]["n_rows"]) and got[0][0]["level"].sum() > 10000


def test_rescaling_job_counts_once_with_its_last_signal(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6106, 12, "rna004", mean, sd, (100, 200))
    sig, seq = [np.ascontiguousarray(1.2 * r.signal + 0.3) for r in reads], [r.sequence for r in reads]
    ids = make_ids(reads, 2)
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_rescale(1)
    al.set_site_summary(NUM_SITES)
    al.set_site_histogram(*SPEC)
    res, xs = run_batch(al, sig, seq, ids)
    assert (res.status == 0).all() and (res.rescale_iters == 1).sum() >= 10
    h = al.site_histogram()
    assert_hist(h, restate_hist(al, res, xs, ids, SPEC))
    assert np.array_equal(h["level"].sum(axis=1), al.site_summary()["n_rows"])       # two passes, counted once
    al.close()


def test_jobs_that_add_nothing_reset_and_the_setters(models):
    """a job without staged ids, a Z-only job and a train job add nothing; bins = 0 stops the counting and keeps the counters;
    reset_site_summary() zeroes them; set_site_summary(0) stops both; set_site_summary(another size) turns the histograms off"""
    reads = polya_reads(models)[:24]
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    ids = make_ids(reads, 21)
    flat = np.concatenate(ids)
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_site_summary(NUM_SITES)
    al.set_site_histogram(*SPEC)
    res, xs = run_batch(al, sig, seq, ids)
    want = restate_hist(al, res, xs, ids, SPEC)
    assert_hist(al.site_histogram(), want, "one job")
    al.align_batch(sig, seq, True)                                   # no ids
    with al.batch(sig, seq, site_ids=flat) as b:
        b.align(False)                                               # Z only
    with al.batch(sig, seq, site_ids=flat) as b:
        b.train()
    assert_hist(al.site_histogram(), want, "after jobs that add nothing")
    al.set_site_histogram(0)                                         # off: the table goes on, the counters stay
    al.align_batch(sig, seq, True, site_ids=flat)
    assert_hist(al.site_histogram(), want, "bins = 0")
    assert int(al.site_summary()["n_rows"].sum()) == 2 * int(np.array(want["level"]).sum())
    al.set_site_histogram(*SPEC)                                     # the same parameters: on again, nothing zeroed
    al.set_site_summary(0)                                           # stops both
    al.align_batch(sig, seq, True, site_ids=flat)
    assert_hist(al.site_histogram(), want, "set_site_summary(0)")
    al.set_site_summary(NUM_SITES)                                   # the same size: the table and the counters as they were
    al.align_batch(sig, seq, True, site_ids=flat)
    twice = {k: (2 * np.array(v, dtype=np.uint32)).tolist() for k, v in want.items()}
    assert_hist(al.site_histogram(), twice, "a second counted job")
    al.reset_site_summary()
    h = al.site_histogram()
    assert not h["level"].any() and not h["dwell"].any() and not al.site_summary()["n_rows"].any()
    al.align_batch(sig, seq, True, site_ids=flat)
    assert_hist(al.site_histogram(), want, "after the reset")
    al.set_site_summary(NUM_SITES // 2)                              # another size: the histograms are released and off
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_histogram\(a, bins > 0, lo, hi\) was never called on this handle"):
        al.site_histogram()
    al.align_batch(sig, seq, True, site_ids=flat)                    # the table alone
    assert al.site_summary()["n_rows"].sum() > 0
    al.set_site_histogram(30, -3.3, 4.1)
    h = al.site_histogram()
    assert h["level"].shape == (NUM_SITES // 2, 32) and not h["level"].any()
    al.close()


def test_setter_with_other_bins_while_a_ticket_is_in_flight(models):
    """the ticket holds the counters it was submitted under: the setter waits for it, then starts zeroed counters"""
    reads = polya_reads(models)
    idx = [i % 48 for i in range(512)]
    ids48 = make_ids(reads, 10)
    packed, flat = synth.pack_reads([reads[i] for i in idx]), np.concatenate([ids48[i] for i in idx])
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_site_summary(NUM_SITES)
    al.set_site_histogram(*SPEC)
    t = al.align_async(*packed, True, site_ids=flat)
    al.set_site_histogram(30, -3.3, 4.1)                             # returns once the ticket is done
    h = al.site_histogram()
    assert h["level"].shape == (NUM_SITES, 32) and not h["level"].any() and not h["dwell"].any()
    res = t.wait()
    assert (res.status == 0).all()
    t.close()
    table = al.site_summary()
    assert table["n_rows"].sum() > 0                                 # the ticket did add to the table it was submitted under
    with al.align_async(*packed, True, site_ids=flat) as t2:
        t2.wait()
    h = al.site_histogram()
    assert np.array_equal(h["level"].sum(axis=1) * 2, al.site_summary()["n_rows"]) and h["level"].sum() > 0
    al.close()


def test_histograms_off_change_no_result_column(models):
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    flat = np.concatenate(make_ids(reads, 8))
    never = Aligner(models["syn5"], "rna002", device=0)              # a handle that never heard of the histograms
    never.set_site_summary(NUM_SITES)
    base = never.align_batch(sig, seq, True, site_ids=flat)
    base_table = never.site_summary()
    never.close()
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_site_summary(NUM_SITES)
    al.set_site_histogram(*SPEC)
    on = al.align_batch(sig, seq, True, site_ids=flat)
    al.set_site_histogram(0)
    al.reset_site_summary()
    off = al.align_batch(sig, seq, True, site_ids=flat)
    m = int(base.seg_offsets[-1])
    for other in (on, off):
        for col in ("Z", "status", "n_segments", "seg_offsets"):
            assert np.asarray(getattr(base, col)).tobytes() == np.asarray(getattr(other, col)).tobytes(), col
        for col in ("signal_positions", "sequence_positions", "probabilities", "states"):
            assert getattr(base, col)[:m].tobytes() == getattr(other, col)[:m].tobytes(), col
    table = al.site_summary()
    assert all(np.array_equal(a, b) for a, b in zip(table["limbs"], base_table["limbs"])) and table["totals"] == base_table["totals"]
    assert not al.site_histogram()["level"].any()                    # zeroed by the reset, untouched since
    al.close()
