"""GPU (-m gpu): per-segment signal levels (Aligner.set_event_stats, event_stats.hip). Every column must equal the NumPy
restatement of the definition BIT FOR BIT on every path that aligns: one launch per batch, merged tickets, resident and
paged sessions, wide bands, strict reads, device preprocessing; switching the levels on must not move a segment or Z."""
import numpy as np
import pytest

from dynamont_amd import Aligner, synth

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


# ---- the definition, restated in NumPy: the oracle of this feature ----
def _chunked(v):
    sums = np.array([np.add.accumulate(v[c:c + 64])[-1] for c in range(0, len(v), 64)])
    return np.add.accumulate(sums)[-1]


def levels_of(x, sp):
    """level_mean / level_stdv / level_median of the segments [sp[i], sp[i+1]) (the last one up to len(x)) of x"""
    x = np.asarray(x, dtype=np.float64)
    bounds = [int(s) for s in sp] + [len(x)]
    out = np.zeros((3, len(sp)))
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        seg = x[a:b]
        L = len(seg)
        mean = _chunked(seg) / np.float64(L)
        d = seg - mean
        stdv = np.sqrt(_chunked(d * d) / np.float64(L))
        s = np.sort(seg)
        med = s[L // 2] if L % 2 else (s[L // 2 - 1] + s[L // 2]) / 2.0
        out[:, i] = (mean, stdv, med + 0.0)
    return out


def check_levels(res, signals, n=None):
    """every ok read's three columns == the restatement over its own signal, bit for bit; returns the segment lengths seen"""
    lengths = []
    for i in range(res.n if n is None else n):
        if res.status[i] != 0:
            continue
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        sp = res.signal_positions[a:b]
        want = levels_of(signals[i], sp)
        got = np.stack([res.level_mean[a:b], res.level_stdv[a:b], res.level_median[a:b]])
        bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=0))
        assert bad.size == 0, (i, bad[:5], got[:, bad[:3]], want[:, bad[:3]])
        lengths += list(np.diff(np.append(sp.astype(np.int64), len(signals[i]))))
    return np.array(lengths)


def same_segments(a, b):
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.Z.view(np.uint64), b.Z.view(np.uint64))
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets)
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "probabilities"):
        assert np.array_equal(getattr(a, col)[:m].view(np.uint64), getattr(b, col)[:m].view(np.uint64)), col


def _model(models, pore):
    return models["syn5"] if pore in ("rna002", "dna_r9") else models["syn9"]


@pytest.mark.parametrize("pore", ["dna_r9", "rna004"])
def test_random_reads_bit_identical_and_switch_changes_nothing_else(models, pore):
    model = _model(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(4101, 40, pore, mean, sd, (60, 400))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(model, pore, device=0)
    off = al.align_batch(sig, seq, True)
    assert off.level_mean is None and "level_mean" not in off.read(0)
    al.set_event_stats(True)
    on = al.align_batch(sig, seq, True)
    same_segments(on, off)
    check_levels(on, sig)
    d = on.read(0)
    assert set(d) >= {"level_mean", "level_stdv", "level_median"} and len(d["level_mean"]) == len(d["signal_positions"])
    again = al.align_batch(sig, seq, True)   # run to run: the same bits
    for col in ("level_mean", "level_stdv", "level_median"):
        assert np.array_equal(getattr(again, col).view(np.uint64), getattr(on, col).view(np.uint64))
    # the single-read surface carries the keys only while the switch is on
    assert "level_median" in al.align(sig[1], seq[1], True)
    al.set_event_stats(False)
    assert "level_median" not in al.align(sig[1], seq[1], True)
    al.close()


def _fixed_dwell_read(rng, mean_c, sd_c, k, dwells, noise=0.05):
    """a read whose k-mers emit for exactly the given dwells, with little noise: the borders land near them"""
    n = len(dwells) + k - 1
    digits = rng.integers(0, 4, size=n)
    codes = synth._seq_codes(digits, k)
    idx = np.repeat(codes, dwells)
    x = mean_c[idx] + noise * sd_c[idx] * rng.standard_normal(len(idx))
    return synth.SynthRead(np.ascontiguousarray(x), "".join(synth.BASES[d] for d in digits))


def test_chunk_and_row_borders_and_stalls(models):
    """dwells around the 64-sample chunks and the 256-row split of the kernels, and stalls of 20 000 / 20 001 samples"""
    pore = "rna004"
    model = _model(models, pore)
    _, mean, sd = synth.read_model_file(model)
    mean_c, sd_c = synth.code_order_table(mean, sd, 9, True)
    rng = np.random.default_rng(77)
    special = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 700]
    reads = []
    for j in range(6):
        dw = np.maximum(2, rng.poisson(10, size=180))
        dw[10::12][:len(special)] = special[:len(dw[10::12])]
        dw[60] = [20000, 20001, 1, 2, 64, 128][j]
        reads.append(_fixed_dwell_read(rng, mean_c, sd_c, 9, dw))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(model, pore, device=0)
    al.set_event_stats(True)
    res = al.align_batch(sig, seq, True)
    assert (res.status == 0).all()
    L = check_levels(res, sig)
    assert L.max() > 10000 and (L % 2 == 0).any() and (L % 2 == 1).any()   # (where the borders land is the aligner's call)
    for lo, hi in ((1, 2), (60, 70), (120, 135), (250, 260), (280, 800)):
        assert ((L >= lo) & (L <= hi)).any(), (lo, hi)
    assert (L > 256).sum() >= 3
    al.close()


def test_wide_band_strict_ties_and_failed_reads(models):
    pore = "rna004"
    model = _model(models, pore)
    _, mean, sd = synth.read_model_file(model)
    wide = synth.make_reads(4201, 6, pore, mean, sd, (600, 900))
    ties = synth.make_reads(4202, 8, pore, mean, sd, (150, 300), polya=(20, 150))
    reads = wide + ties
    reads[3] = synth.SynthRead(reads[3].signal, reads[3].sequence[:40] + "N" + reads[3].sequence[41:])
    reads[9] = synth.SynthRead(reads[9].signal[:50], reads[9].sequence)   # signal too short for the sequence
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(model, pore, band=1000, device=0)
    al.set_event_stats(True)
    res = al.align_batch(sig, seq, True)
    assert res.status[3] != 0 and res.status[9] != 0 and (np.delete(res.status, [3, 9]) == 0).all()
    check_levels(res, sig)
    for i in (3, 9):
        assert res.n_segments[i] == 0
    al.close()


def test_fetch_fails_cleanly_when_not_requested(models):
    pore = "rna004"
    model = _model(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(4301, 5, pore, mean, sd, (60, 200))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    from dynamont_amd import _native as N
    al = Aligner(model, pore, device=0)
    cols = [np.zeros(4096) for _ in range(3)]
    ev = N.DynEventOut(*[c.ctypes.data_as(N.c_double_p) for c in cols], 4096)
    with al.batch(sig, seq) as b:
        b.align(True)                         # switch off at submission
        al.set_event_stats(True)
        with pytest.raises(ValueError, match="without dyn_aligner_set_event_stats"):
            b.fetch_events(ev)
        b.align(False)                        # Z only, switch on
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_events(ev)
        b.align(True)
        b.fetch_events(ev)
    t = al.align_async(*synth.pack_reads(reads), False)
    assert t.wait().level_mean is None
    with pytest.raises(ValueError):
        t.fetch_events(ev)
    t.close()
    al.close()


def test_raw_async_levels_of_the_device_preprocessed_signal(models):
    pore = "rna004"
    model = _model(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(4401, 30, pore, mean, sd, (100, 300))
    rng = np.random.default_rng(3)
    shift = rng.uniform(80, 100, len(reads))
    scale = rng.uniform(10, 20, len(reads))
    raw = [(r.signal * sc + sh).astype(np.float32) for r, sh, sc in zip(reads, shift, scale)]
    seq = [r.sequence for r in reads]
    al = Aligner(model, pore, device=0)
    al.set_event_stats(True)
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
    check_levels(res, aligned)
    t.close()
    al.close()


def test_merged_tickets(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = []
    for j in range(8):
        reads = synth.make_reads(4500 + j, 300, "rna004", mean, sd, (300, 500))
        data.append((reads, synth.pack_reads(reads)))
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_event_stats(True)
    merged = False
    for attempt in range(3):   # (whether tickets meet in the queue is a matter of timing)
        tickets = [al.align_async(*packed, True) for _, packed in data]
        for t, (reads, _) in zip(tickets, data):
            res = t.wait()
            check_levels(res, [r.signal for r in reads])
            merged |= t.timing()["launch_share"] < 1.0
            t.close()
        if merged:
            break
    assert merged
    al.close()


def test_resident_session(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(4600 + j, 600, "rna004", mean, sd, (100, 300)) for j in range(3)]
    al = Aligner(models["syn9"], "rna004", device=0)
    want = [al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True) for reads in data]
    al.set_event_stats(True)
    tickets = [al.align_async(*synth.pack_reads(reads), True) for reads in data]
    for t, reads, w in zip(tickets, data, want):
        res = t.wait()
        assert t.timing()["launches"] == 0        # published into the resident session
        same_segments(res, w)
        check_levels(res, [r.signal for r in reads])
        t.close()
    al.close()


def test_paged_session(models, monkeypatch):
    monkeypatch.setenv("DYN_FORCE_LAYOUT", "separate")
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(4700 + j, 640, "rna004", mean, sd, (100, 420)) for j in range(2)]
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_mem_budget(3 << 30)
    al.set_event_stats(True)
    tickets = [al.align_async(*synth.pack_reads(reads), True) for reads in data]
    for t, reads in zip(tickets, data):
        res = t.wait()
        tm = t.timing()
        assert tm["launches"] == 0 and tm["pool_pages"] < tm["n_waves"] * 8
        check_levels(res, [r.signal for r in reads])
        t.close()
    al.close()
