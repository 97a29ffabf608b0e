"""GPU (-m gpu): the band-margin diagnostics (Aligner.set_band_margin, band_margin.hip) and the re-alignment at a wider band
(Aligner.set_band_retry). Every comparison is of exact integers (tests/band_margin_cases.py restates the definition over all
path rows):
  1. the product's kernels on descriptors and borders of the test's own (tests/device_math/band_margin.hip, built with the
     product's flags), twice, on a read range and on the empty range;
  2. whole reads, the margins restated from the borders the same batch returned: one launch, a resident session with four
     tickets in flight, a merged launch where only some members asked, a wide-band handle, a rescaling job; the switch off
     changes nothing and the fetch says why it fails;
  3. the retry on reads picked on the CPU oracle alone (tests/test_band_margin_host.py).
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import band_margin_cases as bmc
import imperfect_families as fam
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

COLS = ("band_margin_low", "band_margin_high", "band_edge_rows")


# ---- 1. the device harness ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("bmargin") / "libbmargin.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/band_margin.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.bm_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def batch():
    return bmc.build_batch()


FILL = 0xdeadbeef


def run_harness(lib, b, lo=0, hi=None, runs=1):
    n = len(b.reads)
    out = np.zeros(3 * n, dtype=np.uint32)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.bm_run(C.c_int(len(b.read)), p(b.seg_off), p(b.T), p(b.N), p(b.bw), p(b.ratio), p(b.read), C.c_int(n), p(b.status),
                   C.c_uint64(len(b.segrow)), p(b.segrow), C.c_uint32(lo), C.c_uint32(n if hi is None else hi), C.c_int(runs),
                   C.c_uint32(FILL), p(out), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    return out.reshape(3, n)


def assert_margins(got, want, b, what=""):
    bad = np.flatnonzero((got != want).any(axis=0))
    assert bad.size == 0, "%s: reads %s: %s" % (what, bad[:5].tolist(), [(b.reads[i].label, got[:, i].tolist(), want[:, i].tolist())
                                                                        for i in bad[:5]])


def test_device_harness_every_integer(harness, batch):
    """one output row, a clamped half band, bands that cover every column, either edge alone, runs of rows on an edge, both
    slacks 0 on one row, 255 / 256 / 257 / 1 000 output rows, a 20 001-row stall, 100 000-row reads whose products land within
    an ulp of an integer, a failed read between ok reads (tests/test_band_margin_host.py shows that three misreadings of the
    definition each change these integers). Twice, and two launches into the same arrays: the same bits."""
    want = bmc.reference(batch)
    first = run_harness(harness, batch)
    assert_margins(first, want, batch, "run 1")
    assert np.array_equal(run_harness(harness, batch), first)
    assert np.array_equal(run_harness(harness, batch, runs=2), first)


def test_device_harness_read_range_and_empty_range(harness, batch):
    """the reads [2, 9) only (a merged launch whose members did not all ask): the others keep what the arrays held"""
    assert_margins(run_harness(harness, batch, 2, 9), bmc.reference(batch, 2, 9, untouched=FILL), batch, "reads 2..8")
    assert (run_harness(harness, batch, 5, 5) == FILL).all()


# ---- 2. whole reads ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    return fam.write_tables(str(tmp_path_factory.mktemp("bm_tables")), ["syn5", "syn9"])


@pytest.fixture(scope="module")
def squeezed(tables):
    """the 16 reads of rna002_squeezed_band50 (the path leaves the band) and their model"""
    f = fam.FAMILIES[bmc.RETRY_FAMILY]
    return tables[f.table][0], f.pore, fam.reads_of(bmc.RETRY_FAMILY, tables)


def restate(res, signals, band):
    """(3, n) uint32: the definition over the borders the batch returned; NONE, NONE, 0 for a failed read"""
    out = np.zeros((3, res.n), dtype=np.uint32)
    for i in range(res.n):
        out[:, i] = (bmc.NONE, bmc.NONE, 0) if res.status[i] != 0 else bmc.margins_of_result(res, i, len(signals[i]) + 1, band)
    return out


def got(res):
    assert all(getattr(res, c) is not None and getattr(res, c).dtype == np.uint32 and len(getattr(res, c)) == res.n for c in COLS)
    return np.stack([getattr(res, c) for c in COLS])


def assert_same_rows(x, y, n_reads=None):
    m = int(x.seg_offsets[x.n if n_reads is None else n_reads])
    for col in ("Z", "status", "n_segments", "seg_offsets"):
        assert np.asarray(getattr(x, col)).tobytes() == np.asarray(getattr(y, col)).tobytes(), col
    for col in ("signal_positions", "sequence_positions", "probabilities", "states"):
        assert getattr(x, col)[:m].tobytes() == getattr(y, col)[:m].tobytes(), col


@pytest.fixture(scope="module")
def base(squeezed):
    """(a) one launch: a synchronous batch at band 50 with a failed read inside, and its margins restated"""
    model, pore, reads = squeezed
    reads = list(reads)
    reads[2] = synth.SynthRead(reads[2].signal, reads[2].sequence[:40] + "N" + reads[2].sequence[41:])   # fails validation
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(model, pore, band=50, device=0)
    al.set_band_margin(True)
    res = al.align_batch(sig, seq, True)
    al.close()
    return reads, sig, seq, res, restate(res, sig, 50)


def test_one_launch_equals_the_restatement(base):
    reads, sig, seq, res, want = base
    assert res.status[2] != 0 and (np.delete(res.status, 2) == 0).all()
    g = got(res)
    assert np.array_equal(g, want), (g.tolist(), want.tolist())
    assert tuple(g[:, 2]) == (bmc.NONE, bmc.NONE, 0)
    ok = np.delete(np.arange(res.n), 2)
    touched = np.minimum(g[0, ok], g[1, ok]) == 0
    assert touched.sum() >= 4 and (~touched).sum() >= 2 and (g[2, ok][touched] > 0).all() and (g[2, ok][~touched] == 0).all()
    d = res.read(0)
    assert [d[c] for c in COLS] == [int(v) for v in g[:, 0]] and res.band_used is None
    assert isinstance(d["band_margin_low"], int)


def _tickets(reads, n_tickets=4, size=512):
    out = []
    for k in range(n_tickets):
        idx = [(3 * k + j) % len(reads) for j in range(size)]
        out.append((idx, synth.pack_reads([reads[i] for i in idx])))
    return out


def _async(al, tickets, switch=None):
    ts = []
    for k, (_, packed) in enumerate(tickets):
        if switch is not None:
            al.set_band_margin(switch[k])
        ts.append(al.align_async(*packed, True))
    out = []
    for t in ts:
        res = t.wait()
        out.append((t, res, t.timing()))
    return out


def test_resident_session_four_tickets_in_flight(squeezed, base):
    model, pore, _ = squeezed
    reads, _, _, _, want = base
    tickets = _tickets(reads, size=640)                                # (at least 512 ok reads open a session; one in 16 fails)
    al = Aligner(model, pore, band=50, device=0)
    al.set_band_margin(True)
    done = _async(al, tickets)
    assert all(tm["launches"] == 0 for _, _, tm in done)               # all published into the resident session
    for (idx, _), (t, res, _) in zip(tickets, done):
        assert np.array_equal(got(res), want[:, idx])
        t.close()
    st = al.session_stats()
    assert st["tickets"] >= 4 and st["aborted"] == 0                   # the switch threw no ticket out of the session
    al.close()


def test_merged_launch_where_only_some_members_asked(squeezed, base):
    model, pore, _ = squeezed
    reads, _, _, base_res, want = base
    tickets = _tickets(reads)
    al = Aligner(model, pore, band=50, device=0)
    al.set_session_mode(False)
    merged = False
    for attempt in range(3):   # (whether tickets meet in the queue is a matter of timing)
        done = _async(al, tickets, switch=(True, False, True, False))
        for k, ((idx, _), (t, res, _)) in enumerate(zip(tickets, done)):
            if k % 2 == 0:
                assert np.array_equal(got(res), want[:, idx]), (attempt, k)
            else:
                assert res.band_margin_low is None and res.band_margin_high is None and res.band_edge_rows is None
                out = _native.DynBandMarginOut(*(np.zeros(res.n, dtype=np.uint32).ctypes.data_as(_native.c_u32_p) for _ in range(3)), res.n)
                with pytest.raises(ValueError, match=r"submitted without dyn_aligner_set_band_margin\(a, 1\)"):
                    t.fetch_band_margin(out)
            t.close()
        merged |= any(tm["launch_share"] < 1.0 for _, _, tm in done)
        if merged:
            break
    assert merged
    al.close()


def test_wide_band_handle(tables):
    """DNA reads of 470+ bases at band 600: half band 300 > 223, the generic wide-band kernel, beside short reads"""
    path, mean, sd = tables["syn9"]
    pore = "dna_r10_400bps"
    reads = synth.make_reads(7201, 2, pore, mean, sd, 480) + synth.make_reads(7202, 2, pore, mean, sd, (100, 200))
    reads += fam.reads_of("dna_r10_400bps_squeezed_band50", tables)[4:5]                 # ~400 bases, squeezed
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(path, pore, band=600, device=0)
    al.set_band_margin(True)
    res = al.align_batch(sig, seq, True)
    assert (res.status == 0).all()
    g = got(res)
    assert np.array_equal(g, restate(res, sig, 600))
    assert (g[:2, :2] != bmc.NONE).all()                                                 # the wide reads: both edges are real somewhere
    al.close()


def test_rescaling_job_reports_its_last_pass(tables):
    path, mean, sd = tables["syn9"]
    reads = synth.make_reads(6106, 12, "rna004", mean, sd, (100, 200))
    sig, seq = [np.ascontiguousarray(1.2 * r.signal + 0.3) for r in reads], [r.sequence for r in reads]
    plain = Aligner(path, "rna004", band=50, device=0)
    first = plain.align_batch(sig, seq, True)
    plain.close()
    al = Aligner(path, "rna004", band=50, device=0)
    al.set_rescale(1)
    al.set_band_margin(True)
    res = al.align_batch(sig, seq, True)
    assert (res.rescale_iters == 1).sum() >= 6
    m = int(res.seg_offsets[-1])
    assert not np.array_equal(res.signal_positions[:m], first.signal_positions[:m])     # the last pass's borders are not the first's
    g = got(res)
    assert np.array_equal(g, restate(res, sig, 50))                                      # ... and the margins are the last pass's
    assert (g[:2] != bmc.NONE).any()
    al.close()


def test_switch_off_changes_nothing_and_the_fetch_says_why(squeezed, base):
    model, pore, _ = squeezed
    _, sig, seq, on, _ = base
    never = Aligner(model, pore, band=50, device=0)
    never.set_event_stats(True)
    ref = never.align_batch(sig, seq, True)
    never.close()
    al = Aligner(model, pore, band=50, device=0)
    al.set_event_stats(True)
    al.set_band_margin(True)
    with_it = al.align_batch(sig, seq, True)
    al.set_band_margin(False)
    with al.batch(sig, seq) as b:
        b.align(True)
        off = b.fetch()
        out = _native.DynBandMarginOut(*(np.zeros(off.n, dtype=np.uint32).ctypes.data_as(_native.c_u32_p) for _ in range(3)), off.n)
        with pytest.raises(ValueError, match=r"dyn_batch_fetch_band_margin: the batch was submitted without dyn_aligner_set_band_margin\(a, 1\)"):
            b.fetch_band_margin(out)
        al.set_band_margin(True)
        b.align(False)                                                                   # a Z-only job has no path
        with pytest.raises(ValueError, match=r"dyn_batch_fetch_band_margin: the batch was not aligned with calc_probabilities = 1"):
            b.fetch_band_margin(out)
    assert off.band_margin_low is None and off.band_used is None and "band_margin_low" not in off.read(0)
    m = int(ref.seg_offsets[-1])
    for other in (with_it, off, on):
        assert_same_rows(ref, other)
    for other in (with_it, off):
        for col in ("level_mean", "level_stdv", "level_median"):
            assert getattr(ref, col)[:m].tobytes() == getattr(other, col)[:m].tobytes(), col
    al.close()


# ---- 3. the retry --------------------------------------------------------------------------------------------------------------
def _fresh(model, pore, band, sig, seq, event_stats=True):
    al = Aligner(model, pore, band=band, device=0)
    al.set_event_stats(event_stats)
    al.set_band_margin(True)
    res = al.align_batch(sig, seq, True)
    al.close()
    return res


def _read_columns(res, i):
    a, n = int(res.seg_offsets[i]), int(res.n_segments[i])
    rows = {c: getattr(res, c)[a:a + n].tobytes() for c in ("signal_positions", "sequence_positions", "probabilities", "states",
                                                            "level_mean", "level_stdv", "level_median")}
    rows.update({c: int(getattr(res, c)[i]) for c in COLS})
    rows["Z"] = np.float64(res.Z[i]).tobytes()
    return rows


@pytest.mark.parametrize("max_band", [4093, 100])
def test_retry_splices_the_wider_alignment_in_place(squeezed, max_band):
    model, pore, reads = squeezed
    flagged, clean = sorted(bmc.RETRY_FLAGGED), list(bmc.RETRY_CLEAN)
    order = [clean[0], flagged[0], flagged[1], clean[1], flagged[2], clean[2], flagged[3]]   # flagged reads between clean ones
    sig, seq = [reads[i].signal for i in order], [reads[i].sequence for i in order]
    al = Aligner(model, pore, band=50, device=0)
    al.set_event_stats(True)
    al.set_band_retry(bmc.RETRY_MIN_MARGIN, max_band=max_band)
    assert al._band_margin
    res = al.align_batch(sig, seq, True)
    want_band = [min(bmc.RETRY_FLAGGED.get(i, 50), max_band) for i in order]                # as the oracle predicted
    assert res.band_used.dtype == np.uint32 and res.band_used.tolist() == want_band
    fresh = {band: _fresh(model, pore, band, sig, seq) for band in sorted(set(want_band))}
    for k, i in enumerate(order):
        assert _read_columns(res, k) == _read_columns(fresh[want_band[k]], k), (i, want_band[k])
    low_high = np.minimum(res.band_margin_low, res.band_margin_high)
    for k, i in enumerate(order):
        reached = i not in bmc.RETRY_FLAGGED or bmc.RETRY_FLAGGED[i] <= max_band
        assert (low_high[k] >= bmc.RETRY_MIN_MARGIN) == reached, (i, int(low_high[k]))   # at max_band = 100 the chain stops there
    # a ticket reports margins but is never retried
    t = al.align_async(*synth.pack_reads([reads[i] for i in order]), True)
    r = t.wait()
    assert r.band_used is None and _read_columns(r, 1) == _read_columns(fresh[50], 1)
    t.close()
    # off again: the margins stay on, nothing is retried
    al.set_band_retry(0)
    plain = al.align_batch(sig, seq, True)
    assert plain.band_used is None and plain.band_margin_low is not None
    assert all(_read_columns(plain, k) == _read_columns(fresh[50], k) for k in range(len(order)))
    al.close()


def test_retry_refuses_the_kmer_summary(squeezed):
    model, pore, _ = squeezed
    al = Aligner(model, pore, band=50, device=0)
    al.set_kmer_summary(True)
    with pytest.raises(ValueError, match="summed twice"):
        al.set_band_retry(1)
    al.set_kmer_summary(False)
    al.set_band_retry(1)
    with pytest.raises(ValueError, match="summed twice"):
        al.set_kmer_summary(True)
    al.close()
