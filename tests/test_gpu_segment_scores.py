"""GPU (-m gpu): per-border segment scores (Aligner.set_segment_scores, segment_scores.hip). (a) The product's kernels and
launches, compiled into a test unit with the product's flags, run on borders the test chooses; (b) whole reads through
align_batch and the other paths that align. Every output bit equals the NumPy restatement of the definition
(tests/segment_scores_cases.py); NaNs compare by bit pattern. Switching the scores on moves nothing else."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import segment_scores_cases as ssc
from conftest import ROOT, model_for
from dynamont_amd import Aligner, _native, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

COLS = ("median_delta", "mad_delta", "homogeneity")


# ---- (a) the device harness ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("sscore") / "libsscore.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/segment_scores.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.ss_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def batch():
    return ssc.build_batch()


GUARD = 64


def run_harness(lib, b, W, fill=0):
    n_out = b.n_seg + GUARD
    out = np.full(3 * n_out, -7.0)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.ss_run(C.c_int(len(b.read)), p(b.sig_off), p(b.seg_off), p(b.path_off), p(b.T), p(b.N), p(b.read), C.c_int(len(b.status)),
                   p(b.status), C.c_uint64(len(b.sig)), p(b.sig), C.c_uint64(b.rows_total), p(b.pathn), C.c_uint64(b.n_seg),
                   p(b.segrow), C.c_int(W), C.c_int(fill), C.c_uint64(n_out), p(out), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    return out.reshape(3, n_out)


@pytest.mark.parametrize("W", ssc.WINDOWS)
def test_device_harness_every_bit(harness, batch, W):
    """segments of 1 .. 9 samples (NaN), 10 .. 30, trimmed lengths 256 / 257 (the split), stalls of 20 000 / 20 001; borders
    within W of both read ends, a single-segment read, a read shorter than W; quantised, constant, negative, -0.0 and denormal
    samples; failed reads between ok ones; 300 descriptors in a permuted order. The columns start as zeros, as in the product:
    rows of failed reads stay 0. A second run over columns filled with 0xab: every row of an ok read is written (the same
    bits), no other."""
    want = ssc.bits(ssc.reference(batch, W))
    got = run_harness(harness, batch, W)
    for c in range(3):
        g = ssc.bits(got[c])
        bad = np.flatnonzero(g[:batch.n_seg] != want[c])
        assert bad.size == 0, (COLS[c], W, bad[:5], got[c][bad[:5]], want[c][bad[:5]].view(np.float64))
        assert not g[batch.n_seg:].any()                                   # the guard: still the fill
    again = run_harness(harness, batch, W, fill=0xab)
    ok_rows = np.zeros(batch.n_seg, dtype=bool)
    for i, (_, _, sp, status) in enumerate(batch.reads):
        if status == 0:
            ok_rows[int(batch.read_seg_off[i]):int(batch.read_seg_off[i]) + len(sp)] = True
    assert 0 < (~ok_rows).sum() < 60
    for c in range(3):
        g = ssc.bits(again[c])
        assert np.array_equal(g[:batch.n_seg][ok_rows], want[c][ok_rows]), COLS[c]
        assert (g[:batch.n_seg][~ok_rows] == np.uint64(0xabababababababab)).all() and (g[batch.n_seg:] == np.uint64(0xabababababababab)).all()


def test_more_reads_than_one_launch_slice(harness):
    """65 541 descriptors: k_score_window runs a second launch over descriptors 65 535 .. 65 540, reads of three rows of 11 .. 30
    samples. The whole batch bit for bit at W = 8 and W = 64 (k_score_window<8> and <64>); a second launch handed the first
    descriptors again would leave zeros in median_delta and mad_delta of those reads (tests/test_segment_scores_host.py)."""
    b = ssc.build_sliced_batch()
    n = len(b.read)
    assert n == ssc.SLICE + ssc.TAIL
    for W in ssc.SLICED_WINDOWS:
        want = ssc.bits(ssc.reference_sliced(b, W))
        other = ssc.bits(ssc.reference_sliced(b, W, skip_descs=np.arange(ssc.SLICE, n)))
        assert ((other[:2] != want[:2]).sum(axis=1) >= 3 * ssc.TAIL).all()
        got = run_harness(harness, b, W)
        for c in range(3):
            g = ssc.bits(got[c])
            bad = np.flatnonzero(g[:b.n_seg] != want[c])
            assert bad.size == 0, (COLS[c], W, len(bad), bad[:5], got[c][bad[:5]], want[c][bad[:5]].view(np.float64))
            assert not g[b.n_seg:].any()


# ---- (b) whole reads -------------------------------------------------------------------------------------------------------------
def check_scores(res, signals, W, n=None):
    """every ok read's three columns == the restatement over its own aligned signal and returned borders, bit for bit; rows of
    failed reads (none in the row space: n_segments = 0). Returns (rows, rows with a homogeneity, delta rows that are NaN
    beyond each read's first)"""
    rows = finite_h = nan_delta = 0
    for i in range(res.n if n is None else n):
        if res.status[i] != 0:
            continue
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        want = ssc.scores(signals[i], res.signal_positions[a:b], W)
        got = np.stack([getattr(res, c)[a:b] for c in COLS])
        bad = np.flatnonzero((ssc.bits(got) != ssc.bits(want)).any(axis=0))
        assert bad.size == 0, (i, W, bad[:5], got[:, bad[:3]], want[:, bad[:3]])
        rows += b - a
        finite_h += int(np.isfinite(got[2]).sum())
        nan_delta += int((~np.isfinite(got[:2, 1:])).sum())
        assert np.isnan(got[:2, 0]).all()
    return rows, finite_h, nan_delta


def same_segments(a, b):
    """no segment, Z or probability moved (as tests/test_gpu_event_stats.py)"""
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.Z.view(np.uint64), b.Z.view(np.uint64))
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets)
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "probabilities"):
        assert np.array_equal(getattr(a, col)[:m].view(np.uint64), getattr(b, col)[:m].view(np.uint64)), col


def random_reads(models, pore):
    seed, n = ssc.RANDOM_READS[pore]
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    return synth.make_reads(seed, n, pore, mean, sd, (60, 400))


@pytest.mark.parametrize("pore", ["dna_r9", "rna004"])
def test_random_reads_bit_identical_and_switch_changes_nothing_else(models, pore):
    reads = random_reads(models, pore)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(model_for(models, pore), pore, device=0)
    off = al.align_batch(sig, seq, True)
    assert off.median_delta is None and "median_delta" not in off.read(0)
    al.set_event_stats(True)
    lv = al.align_batch(sig, seq, True)
    al.set_segment_scores(8)
    on = al.align_batch(sig, seq, True)
    same_segments(on, off)
    for col in ("level_mean", "level_stdv", "level_median"):                # no level column moved either
        assert np.array_equal(getattr(on, col).view(np.uint64), getattr(lv, col).view(np.uint64)), col
    assert (on.status == 0).all()
    rows, finite_h, nan_delta = check_scores(on, sig, 8)
    # a condition of the inputs (tests/test_segment_scores_host.py confirms it on the CPU oracle's borders for these seeds)
    assert finite_h >= 0.25 * rows and nan_delta == 0
    d = on.read(0)
    assert set(d) >= set(COLS) and all(len(d[c]) == len(d["signal_positions"]) for c in COLS)
    again = al.align_batch(sig, seq, True)                                   # run to run: the same bits
    for col in COLS:
        assert np.array_equal(getattr(again, col).view(np.uint64), getattr(on, col).view(np.uint64))
    al.set_event_stats(False)
    al.set_segment_scores(64)                                                # another window, the levels off
    wide = al.align_batch(sig, seq, True)
    assert wide.level_mean is None
    same_segments(wide, off)
    check_scores(wide, sig, 64)
    # the single-read surface carries the keys only while the switch is on
    one = al.align(sig[1], seq[1], True)
    a = int(wide.seg_offsets[1])
    assert np.array_equal(ssc.bits(one["homogeneity"]), ssc.bits(wide.homogeneity[a:a + len(one["homogeneity"])]))
    al.set_segment_scores(0)
    assert "median_delta" not in al.align(sig[1], seq[1], True)
    al.close()


def test_switch_is_read_at_submission_and_fetch_fails_cleanly(models):
    pore = "rna004"
    reads = random_reads(models, pore)[:6]
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(model_for(models, pore), pore, device=0)
    cols = [np.zeros(4096) for _ in range(3)]
    sc = _native.DynScoreOut(*[c.ctypes.data_as(_native.c_double_p) for c in cols], 4096)
    al.set_segment_scores(5)
    before = al.align_async(*synth.pack_reads(reads), True)                 # submitted with the switch on ...
    al.set_segment_scores(0)
    after = al.align_async(*synth.pack_reads(reads), True)                  # ... and off
    res = before.wait()
    assert res.median_delta is not None
    check_scores(res, sig, 5)
    assert after.wait().median_delta is None
    with pytest.raises(ValueError, match="without dyn_aligner_set_segment_scores"):
        after.fetch_scores(sc)
    same_segments(res, after.result)
    before.close()
    after.close()
    with al.batch(sig, seq) as b:
        b.align(True)                          # switch off at submission
        al.set_segment_scores(5)
        with pytest.raises(ValueError, match="without dyn_aligner_set_segment_scores"):
            b.fetch_scores(sc)
        b.align(False)                         # Z only, switch on
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_scores(sc)
        b.align(True)
        b.fetch_scores(sc)
        small = _native.DynScoreOut(*[c.ctypes.data_as(_native.c_double_p) for c in cols], 3)
        with pytest.raises(ValueError, match="capacity"):
            b.fetch_scores(small)
    al.close()


def test_sink_refuses_a_ticket_submitted_with_the_switch_off(models, tmp_path):
    pore = "rna004"
    reads = random_reads(models, pore)[:4]
    al = Aligner(model_for(models, pore), pore, device=0)
    L = _native.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    assert L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1,
                                  _native.DYN_CSV_SEGMENT_SCORES, C.byref(h), err, 1024) == 0, err.value
    sig, sig_off, seqs, seq_off = synth.pack_reads(reads)
    n = len(reads)
    rid = (C.c_char_p * n)(*[f"r{i}".encode() for i in range(n)])
    sid = (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)])
    starts = np.zeros(n, dtype=np.int64)
    lengths = np.diff(np.asarray(sig_off).astype(np.int64)).astype(np.uint64)
    so = np.ascontiguousarray(seq_off, dtype=np.uint64)

    def submit(t):
        return L.dyn_csv_sink_submit(h, al._h, t._h, C.byref(t.result._c), n, seqs, so.ctypes.data_as(_native.c_u64_p), rid, sid,
                                     starts.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(_native.c_u64_p))

    off = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(off) == _native.DYN_ERR_INVALID_ARGUMENT and "DYN_CSV_SEGMENT_SCORES" in al.last_error()
    al.set_segment_scores(8)
    on = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(on) == 0
    assert L.dyn_csv_sink_wait(h, 1, -1) == 1
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    from dynamont_amd import zstd_io
    lines = zstd_io.decompress(open(tmp_path / "o.csv.zst", "rb").read()).split(b"\n")
    assert lines[0].endswith(b",polish,median_delta,mad_delta,homogeneity")
    res = on.wait()
    assert len(lines) - 2 == int(res.n_segments.sum())
    a = int(res.seg_offsets[0])
    assert lines[1].endswith(",nan,nan,{:.6f}".format(res.homogeneity[a]).encode())
    assert lines[2].endswith(",{:.6f},{:.6f},{:.6f}".format(*(getattr(res, c)[a + 1] for c in COLS)).encode())
    off.wait()
    off.close()
    on.close()
    al.close()


def test_rescaling_and_levels_scored_over_the_last_pass(models):
    pore = "rna004"
    reads = random_reads(models, pore)[:12]
    sig, seq = [np.ascontiguousarray(1.2 * r.signal + 0.3) for r in reads], [r.sequence for r in reads]
    al = Aligner(model_for(models, pore), pore, device=0)
    al.set_rescale(2)
    al.set_event_stats(True)
    al.set_segment_scores(8)
    with al.batch(sig, seq) as b:
        b.align(True)
        res = b.fetch()
        x = b.signals()
    off = np.concatenate([[0], np.cumsum([len(v) for v in sig])]).astype(np.int64)
    xs = [x[int(off[i]):int(off[i + 1])] for i in range(len(sig))]
    assert (res.status == 0).all() and (res.rescale_iters >= 1).sum() >= 8
    assert sum(not np.array_equal(a, s0) for a, s0 in zip(xs, sig)) >= 8     # the signal the last pass aligned is not the input
    check_scores(res, xs, 8)
    assert res.level_mean is not None
    al.close()


def test_wide_band_strict_ties_failed_reads_and_a_stall(models):
    """band 1000 (the wide-band kernel, band_reads.hip) with polyA reads (strict tie rows), two reads that fail, and a read with a stalled pore"""
    pore = "rna004"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    mean_c, sd_c = synth.code_order_table(mean, sd, 9, True)
    wide = synth.make_reads(7201, 2, pore, mean, sd, (600, 700))
    ties = synth.make_reads(7202, 5, pore, mean, sd, (150, 300), polya=(20, 150))
    rng = np.random.default_rng(73)
    dw = np.maximum(2, rng.poisson(10, size=120))
    dw[40], dw[70], dw[90] = 20000, 321, 700
    n = len(dw) + 8
    digits = rng.integers(0, 4, size=n)
    idx = np.repeat(synth._seq_codes(digits, 9), dw)
    stalled = synth.SynthRead(np.ascontiguousarray(mean_c[idx] + 0.05 * sd_c[idx] * rng.standard_normal(len(idx))),
                              "".join(synth.BASES[d] for d in digits))
    reads = wide + ties + [stalled]
    reads[1] = synth.SynthRead(reads[1].signal, reads[1].sequence[:40] + "N" + reads[1].sequence[41:])
    reads[4] = synth.SynthRead(reads[4].signal[:50], reads[4].sequence)      # signal too short for the sequence
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(model, pore, band=1000, device=0)
    off = al.align_batch(sig, seq, True)
    al.set_segment_scores(8)
    res = al.align_batch(sig, seq, True)
    same_segments(res, off)
    assert res.status[1] != 0 and res.status[4] != 0 and (np.delete(res.status, [1, 4]) == 0).all()
    check_scores(res, sig, 8)
    a, m = int(res.seg_offsets[7]), int(res.n_segments[7])
    L = np.diff(np.append(res.signal_positions[a:a + m].astype(np.int64), len(sig[7])))
    assert L.max() > 10000 and (L > 330).sum() >= 2                          # the radix select ran
    al.close()


def test_band_600_read(models):
    pore = "dna_r10_400bps"
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(7204, 1, pore, mean, sd, 480) + synth.make_reads(7205, 2, pore, mean, sd, (100, 200))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn9"], pore, band=600, device=0)
    al.set_segment_scores(16)
    res = al.align_batch(sig, seq, True)
    assert (res.status == 0).all()
    check_scores(res, sig, 16)
    al.close()


def test_resident_session_of_short_reads(models):
    """tickets of 600 short reads: the resident session opens; each ticket's scores follow its own borders"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(7300 + j, 600, "rna004", mean, sd, (60, 120)) for j in range(2)]
    al = Aligner(models["syn9"], "rna004", device=0)
    want = [al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True) for reads in data]
    al.set_segment_scores(8)
    tickets = [al.align_async(*synth.pack_reads(reads), True) for reads in data]
    for t, reads, w in zip(tickets, data, want):
        res = t.wait()
        assert t.timing()["launches"] == 0        # published into the resident session
        same_segments(res, w)
        check_scores(res, [r.signal for r in reads], 8, n=150)
        t.close()
    st = al.session_stats()
    assert st["tickets"] >= 2 and st["aborted"] == 0
    al.close()


def test_raw_int16_input(models):
    pore = "rna004"
    reads = random_reads(models, pore)
    rng = np.random.default_rng(3)
    shift = rng.uniform(400, 500, len(reads))
    scale = rng.uniform(60, 90, len(reads))
    raw = [np.round(r.signal * sc + sh).astype(np.int16) for r, sh, sc in zip(reads, shift, scale)]
    seq = [r.sequence for r in reads]
    al = Aligner(model_for(models, pore), pore, device=0)
    al.set_segment_scores(8)
    with al.batch_raw(raw, seq, shift, scale) as b:
        x = b.signals()
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in raw])
    aligned = [x[int(off[i]):int(off[i + 1])] for i in range(len(raw))]
    seqs = "".join(seq).encode()
    seq_off = np.zeros(len(seq) + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seq])
    t = al.align_raw_async(np.concatenate(raw), off, shift, scale, seqs, seq_off)
    res = t.wait()
    assert (res.status == 0).all()
    check_scores(res, aligned, 8)
    t.close()
    al.close()
