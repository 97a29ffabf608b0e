"""GPU (-m gpu): P1/P2 on the device (dyn_batch_create_raw) is bit-identical to the NumPy
preprocessing of the reference's workers (segment.py:146-153 float64 / train.py:163-170 float32),
whose `hampel` is itself pinned to the reference's outputs in tests/test_harness.py.
The kernels themselves, every instantiation and window: tests/test_gpu_preprocess_kernels.py. Here: the product's entry
points -- synchronous raw batches, raw / VBZ / training tickets, merged raw tickets."""
import numpy as np
import pytest

from conftest import model_for
from dynamont_amd import Aligner, synth
from dynamont_amd._dynamont import Batch
from dynamont_amd.segmentation.utils import hampel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


def _numpy_prep(raw, shift, scale, W, ns, f32):
    x = np.array(raw, dtype=np.float32 if f32 else np.float64, copy=True)
    x -= shift
    x /= scale
    hampel(x, W, ns)
    return x.astype(np.float64)


@pytest.mark.parametrize("dtype,W,ns,f32", [(np.float32, 3, 3.0, False), (np.int16, 3, 3.0, False),
                                            (np.float32, 7, 5.0, True), (np.float64, 4, 3.0, False)])
def test_device_preprocessing_bit_identical(models, dtype, W, ns, f32):
    rng = np.random.default_rng(7)
    al = Aligner(models["syn5"], "dna_r9", device=0)
    raws, seqs, shifts, scales = [], [], [], []
    for size in (0, 1, W - 1, W, W + 1, W + 2, 57, 1000, 20011):
        pa = rng.normal(90.0, 15.0, size)
        if size > 20:
            pa[rng.integers(0, size, size=max(1, size // 20))] += rng.choice([-70.0, 55.0, 200.0])
            pa[5:9] = pa[5]                                        # flat run: MAD == 0
        raw = np.rint(pa * 5.7).astype(np.int16) if dtype == np.int16 else pa.astype(dtype)
        raws.append(raw)
        seqs.append("ACGTACGTAC")
        shifts.append(float(np.float32(rng.uniform(80, 100))) * (5.7 if dtype == np.int16 else 1.0))
        scales.append(float(np.float32(rng.uniform(10, 20))))
    with al.batch_raw(raws, seqs, shifts, scales, window=W, n_sigmas=ns, f32=f32) as b:
        got = b.signals()
    want = np.concatenate([_numpy_prep(r, sh, sc, W, ns, f32) for r, sh, sc in zip(raws, shifts, scales)])
    assert got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.any(np.concatenate([_numpy_prep(r, sh, sc, W, 1e9, f32) for r, sh, sc in zip(raws, shifts, scales)]) != want)


def test_raw_batch_alignment_equals_host_preprocessed(models):
    """align on a raw batch == align on the host-preprocessed signals (same kernels, same inputs)."""
    pore = "rna004"
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    reads = synth.make_reads(81, 6, pore, mean, sd, (100, 400))
    al = Aligner(model_for(models, pore), pore, device=0)
    raws = [(r.signal * 15.0 + 90.0).astype(np.float32) for r in reads]
    shifts, scales = [90.0] * len(reads), [15.0] * len(reads)
    seqs = [r.sequence for r in reads]
    host = al.align_batch([_numpy_prep(x, 90.0, 15.0, 3, 3.0, False) for x in raws], seqs, True)
    with al.batch_raw(raws, seqs, shifts, scales) as b:
        b.align(True)
        dev = b.fetch()
    for i in range(len(reads)):
        a, c = host.read(i), dev.read(i)
        assert a["Z"] == c["Z"] and np.array_equal(a["signal_positions"], c["signal_positions"])
        assert np.array_equal(a["probabilities"], c["probabilities"])


def _pack(raws, seqs):
    off = np.zeros(len(raws) + 1, dtype=np.uint64)
    so = np.zeros(len(raws) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raws], out=off[1:])
    np.cumsum([len(s) for s in seqs], out=so[1:])
    return np.concatenate(raws), off, "".join(seqs).encode(), so


@pytest.mark.parametrize("calibrated", [True, False])
def test_raw_async_equals_host_preprocessed(models, calibrated):
    """dyn_batch_align_raw_async (what dynamont-resquiggle drives): int16 ADC counts, with the pod5 calibration
    (picoampere formed on the device, raw_dtype 3) or without it (raw_dtype 1), three batches in flight -- every
    result bit-identical to the synchronous call on signals preprocessed with NumPy the way segment.py:141-153 does."""
    pore = "rna004"
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    al = Aligner(model_for(models, pore), pore, device=0)
    rng = np.random.default_rng(5)
    tickets, wants = [], []
    for j in range(4):
        reads = synth.make_reads(500 + j, 9, pore, mean, sd, (60, 300))
        seqs = [r.sequence for r in reads]
        cal_off = rng.uniform(-260, -200, len(reads)).astype(np.float32)
        cal_sc = rng.uniform(0.15, 0.2, len(reads)).astype(np.float32)
        adcs = [np.rint((r.signal * 15.0 + 90.0) / float(sc) - float(of)).astype(np.int16) for r, of, sc in zip(reads, cal_off, cal_sc)]
        if calibrated:
            shifts, scales = rng.uniform(85, 95, len(reads)), rng.uniform(13, 17, len(reads))
            host = [_numpy_prep((a.astype(np.float32) + of) * sc, sh, sc2, 3, 3.0, False)
                    for a, of, sc, sh, sc2 in zip(adcs, cal_off, cal_sc, shifts, scales)]
        else:  # shift > 400: the reference takes the ADC counts themselves (segment.py:147)
            shifts, scales = rng.uniform(700, 800, len(reads)), rng.uniform(80, 100, len(reads))
            host = [_numpy_prep(a, sh, sc2, 3, 3.0, False) for a, sh, sc2 in zip(adcs, shifts, scales)]
        wants.append(al.align_batch(host, seqs, True))
        raw, off, sq, so = _pack(adcs, seqs)
        # odd batches: the slices as a list (DYN_RAW_SCATTERED: the library gathers them), even ones concatenated
        tickets.append(al.align_raw_async(adcs if j % 2 else raw, off, shifts, scales, sq, so,
                                          calibration=(cal_off, cal_sc) if calibrated else None))
    for t, want in zip(tickets, wants):
        got = t.wait()
        assert np.array_equal(got.status, want.status) and (got.status == 0).all()
        for i in range(got.n):
            a, c = want.read(i), got.read(i)
            assert a["Z"] == c["Z"] and np.array_equal(a["signal_positions"], c["signal_positions"])
            assert np.array_equal(a["probabilities"], c["probabilities"])
        t.close()


def test_train_raw_async_equals_host_preprocessed(models):
    """dyn_batch_train_raw_async: float32 arithmetic + Hampel(7, 5 sigma) as in train.py:163-170."""
    pore = "rna002"
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    al = Aligner(model_for(models, pore), pore, device=0)
    reads = synth.make_reads(77, 5, pore, mean, sd, (60, 200))
    seqs = [r.sequence for r in reads]
    raws = [(r.signal * 15.0 + 90.0).astype(np.float32) for r in reads]
    host = al.train_batch([_numpy_prep(x, 90.0, 15.0, 7, 5.0, True) for x in raws], seqs)
    raw, off, sq, so = _pack(raws, seqs)
    t = al.train_raw_async(raw, off, [90.0] * len(reads), [15.0] * len(reads), sq, so)
    got = t.wait()
    assert np.array_equal(got.Z, host.Z) and np.array_equal(got.transitions, host.transitions)
    for i in range(len(reads)):
        for x, y in zip(got.sparse(i), host.sparse(i)):
            assert np.array_equal(x, y)
    t.close()


# ---- the product's entry points, every variant ---------------------------------------------------------------------------------
# dyn_batch_signals serves a ticket after wait() and before close(), merged launch or not (AsyncBatch.signals): below the
# SIGNAL ITSELF is compared with the NumPy restatement, and Z, borders and probabilities with the synchronous call on it.
VARIANTS = ["calibrated", "uncalibrated", "f32_picoampere"]
LEAD_RAW, LEAD_SEQ = 37, 11   # samples / characters in front of the first read: the first offsets are not 0


def _pa(adc, off, sc):
    """pod5's signal_pa: float32, one operation each"""
    return (adc.astype(np.float32) + np.float32(off)) * np.float32(sc)


def _make_raw(reads, variant, rng, k=0):
    """(raw slices, shift, scale, calibration or None) of one ticket, every read its own values, ranges that move with k"""
    n = len(reads)
    cal_off = rng.uniform(-260 + 5 * k, -255 + 5 * k, n).astype(np.float32)
    cal_sc = rng.uniform(0.15 + 0.005 * k, 0.155 + 0.005 * k, n).astype(np.float32)
    pa = [r.signal * 15.0 + 90.0 for r in reads]
    if variant == "f32_picoampere":
        return [x.astype(np.float32) for x in pa], rng.uniform(85 + k, 86 + k, n), rng.uniform(13 + 0.4 * k, 13.4 + 0.4 * k, n), None
    adcs = [np.rint(x / float(sc) - float(of)).astype(np.int16) for x, of, sc in zip(pa, cal_off, cal_sc)]
    if variant == "calibrated":
        return adcs, rng.uniform(85 + k, 86 + k, n), rng.uniform(13 + 0.4 * k, 13.4 + 0.4 * k, n), (cal_off, cal_sc)
    # shift > 400: the reference takes the ADC counts themselves (segment.py:147)
    return adcs, rng.uniform(700 + 10 * k, 710 + 10 * k, n), rng.uniform(80 + 2 * k, 82 + 2 * k, n), None


def _host(raws, shifts, scales, cal, W=3, ns=3.0, f32=False):
    if cal is not None:
        raws = [_pa(a, of, sc) for a, of, sc in zip(raws, cal[0], cal[1])]
    return [_numpy_prep(x, float(sh), float(sc), W, ns, f32) for x, sh, sc in zip(raws, shifts, scales)]


def _pack_with_lead(raws, seqs):
    """_pack with LEAD_RAW samples and LEAD_SEQ characters that belong to no read in front"""
    raw, off, sq, so = _pack(raws, seqs)
    junk = np.full(LEAD_RAW, 12345 if raw.dtype == np.int16 else 1e4, dtype=raw.dtype)
    return np.concatenate([junk, raw]), off + np.uint64(LEAD_RAW), b"N" * LEAD_SEQ + sq, so + np.uint64(LEAD_SEQ)


def _same_alignment(got, want):
    assert np.array_equal(got.status, want.status)
    for i in range(want.n):
        if want.status[i] != 0:
            continue
        a, c = want.read(i), got.read(i)
        assert a["Z"] == c["Z"] and np.array_equal(a["signal_positions"], c["signal_positions"]), i
        assert np.array_equal(a["probabilities"], c["probabilities"]), i


@pytest.mark.parametrize("form", ["concatenated", "slices"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_raw_ticket_signal_every_variant(models, variant, form):
    """align_raw_async: int16 + calibration (raw_dtype 3), int16 alone (1), float32 picoampere (0); the batch concatenated
    (first raw offset 37, first sequence offset 11) and as a list of slices."""
    pore = "rna004"
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    al = Aligner(model_for(models, pore), pore, device=0)
    reads = synth.make_reads(900 + VARIANTS.index(variant), 9, pore, mean, sd, (60, 300))
    seqs = [r.sequence for r in reads]
    raws, shifts, scales, cal = _make_raw(reads, variant, np.random.default_rng(11))
    host = _host(raws, shifts, scales, cal)
    want = al.align_batch(host, seqs, True)
    if form == "concatenated":
        raw, off, sq, so = _pack_with_lead(raws, seqs)
        assert off[0] == LEAD_RAW and so[0] == LEAD_SEQ
    else:
        (_, off, sq, so), raw = _pack(raws, seqs), raws
    t = al.align_raw_async(raw, off, shifts, scales, sq, so, calibration=cal)
    got = t.wait()
    x = t.signals(sum(len(r) for r in raws))
    assert np.array_equal(x, np.concatenate(host))
    assert (got.status == 0).all()
    _same_alignment(got, want)
    t.close()
    al.close()


@pytest.mark.parametrize("dtype", [np.float32, np.int16, np.float64])
def test_sync_raw_batch_with_first_offsets_other_than_zero(models, dtype):
    """Batch(..., raw=...) (dyn_batch_create_raw) on arrays whose first raw offset is 37 and first sequence offset 11."""
    pore = "rna004"
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    al = Aligner(model_for(models, pore), pore, device=0)
    reads = synth.make_reads(930, 6, pore, mean, sd, (60, 300))
    seqs = [r.sequence for r in reads]
    raws, shifts, scales, _ = _make_raw(reads, "uncalibrated" if dtype == np.int16 else "f32_picoampere", np.random.default_rng(12))
    if dtype == np.float64:
        raws = [r.signal * 15.0 + 90.0 for r in reads]      # (not float32 values widened)
    assert all(x.dtype == dtype for x in raws)
    host = _host(raws, shifts, scales, None)
    want = al.align_batch(host, seqs, True)
    raw, off, sq, so = _pack_with_lead(raws, seqs)
    with Batch(al, raw, off, sq, so, raw=dict(shift=shifts, scale=scales, window=3, n_sigmas=3.0, f32=False)) as b:
        assert np.array_equal(b.signals(), np.concatenate(host))
        b.align(True)
        _same_alignment(b.fetch(), want)
    al.close()


def test_train_raw_async_with_calibration(models):
    """train_raw_async(int16, calibration=...) at f32=True (float/int16+calibration): picoampere in float32, float32
    normalisation, Hampel(7, 5 sigma) -- Z, transitions, sparse statistics and pooled sums of train_batch on the
    host-preprocessed float32 signal, bit for bit; first offsets 37 and 11."""
    pore = "rna002"
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    al = Aligner(model_for(models, pore), pore, device=0)
    reads = synth.make_reads(78, 5, pore, mean, sd, (60, 200))
    seqs = [r.sequence for r in reads]
    raws, shifts, scales, cal = _make_raw(reads, "calibrated", np.random.default_rng(13))
    host = _host(raws, shifts, scales, cal, 7, 5.0, True)
    assert any(np.any(a != b) for a, b in zip(host, _host(raws, shifts, scales, cal, 7, 5.0, False)))   # float32 is not float64 here
    want = al.train_batch(host, seqs, pooled=True)
    raw, off, sq, so = _pack_with_lead(raws, seqs)
    t = al.train_raw_async(raw, off, shifts, scales, sq, so, pooled=True, calibration=cal)
    got = t.wait()
    assert np.array_equal(t.signals(sum(len(r) for r in raws)), np.concatenate(host))
    assert (got.status == 0).all() and np.array_equal(got.status, want.status)
    assert np.array_equal(got.Z, want.Z) and np.array_equal(got.transitions, want.transitions)
    assert np.array_equal(got.trans_counts, want.trans_counts)
    for i in range(len(reads)):
        for x, y in zip(got.sparse(i), want.sparse(i)):
            assert np.array_equal(x, y)
        a, b = int(want.em_offsets[i]), int(want.em_offsets[i]) + int(want.em_count[i])
        ga = int(got.em_offsets[i])
        for name in ("em_weight", "em_sum", "em_sumsq"):
            assert np.array_equal(getattr(got, name)[ga:ga + b - a], getattr(want, name)[a:b]), name
    assert np.array_equal(got.pooled, want.pooled) and np.any(want.pooled != 0)
    t.close()
    al.close()


@pytest.fixture(scope="module")
def merge_reads(models):
    """eight tickets of 300 reads (the shape of test_waiting_tickets_share_one_launch), made once for both variants"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    return [synth.make_reads(1700 + j, 300, "rna004", mean, sd, (300, 500)) for j in range(8)]


@pytest.mark.parametrize("variant,form", [("calibrated", "concatenated"), ("uncalibrated", "slices")])
def test_merged_raw_tickets(models, merge_reads, monkeypatch, variant, form):
    """Pipeline::merge on RAW tickets (what dynamont-resquiggle produces under load): tickets that wait while the GPU is
    busy share a launch, their per-read shift, scale and calibration are concatenated and their samples become scattered
    pointers. Every ticket has its own ranges of shift, scale and calibration; one more ticket differs from ticket 0 only
    in `window` and must run alone. Every ticket's signal equals the NumPy restatement and its results the synchronous call
    on that signal. With DYN_NO_MERGE=1: the same, every launch_share 1."""
    al = Aligner(models["syn9"], "rna004", device=0)
    data = []
    for j, reads in enumerate(merge_reads + [merge_reads[0]]):
        W = 5 if j == 8 else 3
        seqs = [r.sequence for r in reads]
        raws, shifts, scales, cal = _make_raw(reads, variant, np.random.default_rng(40 + j), k=j % 8)
        host = _host(raws, shifts, scales, cal, W)
        args = _pack_with_lead(raws, seqs) if form == "concatenated" else (raws,) + _pack(raws, seqs)[1:]
        data.append(dict(W=W, host=np.concatenate(host), want=al.align_batch(host, seqs, True), args=args,
                         kw=dict(window=W, calibration=cal), shifts=shifts, scales=scales))
    assert np.any(data[8]["host"] != data[0]["host"])      # window 5 is not window 3 on these reads
    order = [0, 1, 2, 3, 8, 4, 5, 6, 7]                    # the other window in the middle of the queue

    def submit(d):
        raw, off, sq, so = d["args"]
        return al.align_raw_async(raw, off, d["shifts"], d["scales"], sq, so, **d["kw"])

    def check(t, d):
        got = t.wait()
        assert np.array_equal(t.signals(d["host"].size), d["host"])
        assert (got.status == 0).all()
        _same_alignment(got, d["want"])
        return t.timing()["launch_share"]

    for attempt in range(3):   # (whether tickets meet in the queue is a matter of timing, as in test_waiting_tickets_share_one_launch)
        tickets = [submit(data[j]) for j in order]
        shares = [check(t, data[j]) for t, j in zip(tickets, order)]
        for t in tickets:
            t.close()
        assert shares[order.index(8)] == 1.0               # never merged: no other ticket has its window
        merged = sum(1 for x in shares if x < 1.0)
        if merged >= 2:
            break
    assert merged >= 2, shares
    al.close()
    monkeypatch.setenv("DYN_NO_MERGE", "1")
    al = Aligner(models["syn9"], "rna004", device=0)
    sub = [0, 1, 8, 2, 3]
    tickets = [submit(data[j]) for j in sub]
    for t, j in zip(tickets, sub):
        assert check(t, data[j]) == 1.0
        t.close()
    al.close()


def test_vbz_tickets_below_the_cli(models):
    """align_vbz_async: POD5 chunks still VBZ-compressed (pod5_native.vbz_compress), reads of one and of several chunks,
    chunk sizes around the 8-value key groups of svb16, a slice that starts inside the first chunk and ends before the last
    one does; with and without calibration the results are those of align_raw_async on the decoded slices. A read whose chunk
    is truncated ends with DYN_READ_BAD_SIGNAL (10) and leaves every other read's result as it was."""
    from dynamont_amd.pod5_native import vbz_compress, vbz_decompress
    pore = "rna004"
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    al = Aligner(model_for(models, pore), pore, device=0)
    reads = synth.make_reads(960, 8, pore, mean, sd, (60, 300))
    seqs = [r.sequence for r in reads]
    rng = np.random.default_rng(14)
    adcs, shifts, scales, cal = _make_raw(reads, "calibrated", rng)
    chunk_sizes = [[None], [7, None], [8, 9, None], [15, 16, 17, None], [1, 64, None], [63, 65, None], [None], [24, 23, None]]
    before, after = [0, 3, 8, 13, 1, 70, 5, 0], [0, 4, 0, 9, 2, 0, 17, 6]     # samples of the read's signal outside the slice
    blobs, nbytes, samples, read_off, skip = [], [], [], [0], []
    for i, a in enumerate(adcs):
        whole = np.concatenate([rng.integers(300, 900, before[i]).astype(np.int16), a, rng.integers(300, 900, after[i]).astype(np.int16)])
        pos = 0
        for size in chunk_sizes[i]:
            part = whole[pos:] if size is None else whole[pos:pos + size]
            pos += len(part)
            blob = vbz_compress(part)
            assert np.array_equal(vbz_decompress(blob, len(part)), part)
            blobs.append(np.frombuffer(blob, dtype=np.uint8).copy())
            nbytes.append(len(blob))
            samples.append(len(part))
        read_off.append(len(blobs))
        skip.append(before[i])
    assert skip[5] > chunk_sizes[5][0] and after[3] > 0       # a slice that starts behind the first chunk; one that ends early
    _, off, sq, so = _pack(adcs, seqs)
    off, sq, so = off + np.uint64(LEAD_RAW), b"N" * LEAD_SEQ + sq, so + np.uint64(LEAD_SEQ)   # (only differences of off are read)
    bad = 3
    for calibration, sh, sc in ((cal, shifts, scales), (None, rng.uniform(700, 800, len(reads)), rng.uniform(80, 100, len(reads)))):
        t0 = al.align_raw_async(adcs, off, sh, sc, sq, so, calibration=calibration)
        want = t0.wait()
        want_x = t0.signals(int(off[-1] - off[0]))
        assert (want.status == 0).all()
        for broken in (False, True):
            use = list(blobs)
            nb = list(nbytes)
            if broken:
                c = read_off[bad] + 1                                              # the second of the read's four chunks
                nb[c] = nb[c] // 2
                use[c] = use[c][:nb[c]].copy()
            ptrs = np.array([x.ctypes.data for x in use], dtype=np.uint64)
            t = al.align_vbz_async((ptrs, nb, samples, read_off, skip), off, sh, sc, sq, so, calibration=calibration)
            got = t.wait()
            x = t.signals(int(off[-1] - off[0]))
            keep = np.ones(len(x), dtype=bool)
            if broken:
                assert got.status[bad] == 10 and (np.delete(got.status, bad) == 0).all()
                lo, hi = int(off[bad] - off[0]), int(off[bad + 1] - off[0])
                keep[lo:hi] = False
            else:
                assert (got.status == 0).all()
            assert np.array_equal(x[keep], want_x[keep])
            for i in range(len(reads)):
                if broken and i == bad:
                    continue
                a, c = want.read(i), got.read(i)
                assert a["Z"] == c["Z"] and np.array_equal(a["signal_positions"], c["signal_positions"]), i
                assert np.array_equal(a["probabilities"], c["probabilities"]), i
            t.close()
            del use
        t0.close()
    al.close()
