"""GPU (-m gpu): per-read signal rescaling (Aligner.set_rescale, rescale.hip). With K iterations every read is aligned
K + 1 times with a GPU refit of its shift and scale between the passes; shift, scale, fits applied, the integer columns and
the aligned signal must equal the NumPy restatement driven through the CPU oracle (tests/rescale_chain.py) BIT FOR BIT, on
every path that aligns; with the switch off nothing moves."""
import numpy as np
import pytest

from dynamont_amd import Aligner, synth
from dynamont_amd import _native as N
from oracle.pyoracle import Oracle
from rescale_chain import (DISTORTIONS, RECOVERY_AGREEMENT, RECOVERY_ITERS, RECOVERY_PARAM_TOL, border_agreement, fit,
                           levels_of, rescale_chain, row_model_means, segment_means)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib", "oracle_built")]

PROB_TOL = 1e-6   # tests/test_gpu_parity.py: PROB_TIGHT
Z_REL = 1e-9
PORES = ["rna004", "dna_r10_400bps"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _slices(sig_lens):
    off = np.concatenate([[0], np.cumsum(sig_lens)]).astype(np.int64)
    return [slice(int(off[i]), int(off[i + 1])) for i in range(len(sig_lens))]


def run_batch(al, sig, seq, calc=True):
    """sync align_batch that also returns the device-resident signal of every read"""
    with al.batch(sig, seq) as b:
        b.align(calc)
        res = b.fetch()
        x = b.signals()
    return res, [x[s] for s in _slices([len(v) for v in sig])]


def same_results(a, b, levels=False, rescale=False):
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(_bits(a.Z), _bits(b.Z))
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets)
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "states"):
        assert np.array_equal(getattr(a, col)[:m], getattr(b, col)[:m]), col
    assert np.array_equal(_bits(a.probabilities[:m]), _bits(b.probabilities[:m]))
    if levels:
        for col in ("level_mean", "level_stdv", "level_median"):
            assert np.array_equal(_bits(getattr(a, col)[:m]), _bits(getattr(b, col)[:m])), col
    if rescale:
        assert np.array_equal(_bits(a.rescale_shift), _bits(b.rescale_shift))
        assert np.array_equal(_bits(a.rescale_scale), _bits(b.rescale_scale))
        assert np.array_equal(a.rescale_iters, b.rescale_iters)


def check_chain(res, xs, chains, K, idx=None):
    """read i of the batch against record K of its restated chain: transforms, integer columns and x_K bit for bit,
    Z and posteriors to the parity suite's tolerances, status and message"""
    for i in (range(res.n) if idx is None else idx):
        rec = chains[i][K]
        assert res.rescale_iters[i] == rec["iters_applied"], i
        assert _bits(res.rescale_shift[i]) == _bits(rec["shift"]) and _bits(res.rescale_scale[i]) == _bits(rec["scale"]), \
            (i, res.rescale_shift[i], rec["shift"], res.rescale_scale[i], rec["scale"])
        if xs is not None:
            assert np.array_equal(_bits(xs[i]), _bits(rec["x"])), i
        if rec["res"] is None:
            assert res.status[i] != 0 and res.error(i) == rec["error"], i
            continue
        got, want = res.read(i), rec["res"]
        assert np.array_equal(got["signal_positions"], want["signal_positions"]), i
        assert np.array_equal(got["sequence_positions"], want["sequence_positions"]), i
        assert got["states"] == want["states"], i
        assert np.abs(got["probabilities"] - want["probabilities"]).max() <= PROB_TOL, i
        assert abs(got["Z"] - want["Z"]) <= Z_REL * max(1.0, abs(want["Z"])), i


def _chains(model, pore, sig, seq, K, band=400):
    orc = Oracle(model, synth.PORES[pore][0], band)
    mm, _ = orc.table()
    k = synth.PORES[pore][2]
    out = []
    for s, q in zip(sig, seq):
        try:
            km = orc.kmers(q)
        except RuntimeError:
            km = np.zeros(0, dtype=np.int32)
        out.append(rescale_chain(lambda x, qq: orc.align(x, qq, True), s, q, mm, km, k, K))
    return out


@pytest.fixture(scope="module")
def parity_data(models):
    """per pore: 48 reads per distortion plus 48 undistorted ones, and their chains up to K = 3"""
    data = {}
    for j, pore in enumerate(PORES):
        _, mean, sd = synth.read_model_file(models["syn9"])
        reads = synth.make_reads(7300 + j, 48, pore, mean, sd, (60, 200))
        sig, seq, clean = [], [], []
        for bb, aa in [(1.0, 0.0)] + DISTORTIONS:
            for r in reads:
                sig.append(np.ascontiguousarray(r.signal if bb == 1.0 else bb * r.signal + aa))
                seq.append(r.sequence)
                clean.append(r.signal)
        data[pore] = (sig, seq, clean, _chains(models["syn9"], pore, sig, seq, 3))
    return data


def test_off_is_off(models, parity_data):
    sig, seq, _, _ = parity_data["rna004"]
    ref = Aligner(models["syn9"], "rna004", device=0)
    ref.set_event_stats(True)
    want, xw = run_batch(ref, sig, seq)
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_event_stats(True)
    al.set_rescale(2)
    al.set_rescale(0)
    got, xg = run_batch(al, sig, seq)
    same_results(got, want, levels=True)
    assert got.rescale_shift is None and "rescale_shift" not in got.read(0)
    for a, b in zip(xg, xw):
        assert np.array_equal(_bits(a), _bits(b))
    ref.close()
    al.close()


@pytest.mark.parametrize("pore", PORES)
@pytest.mark.parametrize("strict", ["ties", "all", "off"])
def test_parity_with_the_chain(models, parity_data, pore, strict):
    sig, seq, _, chains = parity_data[pore]
    al = Aligner(models["syn9"], pore, device=0)
    al.set_strict(strict)
    for K in (1, 3):
        al.set_rescale(K)
        res, xs = run_batch(al, sig, seq)
        assert (res.status == 0).all()
        check_chain(res, xs, chains, K)
        d = res.read(5)
        assert {"rescale_shift", "rescale_scale", "rescale_iters"} <= set(d)
        if K == 3:
            assert (res.rescale_iters[48:] >= 1).all()   # every distorted read was refitted
    al.close()


def test_determinism(models, parity_data):
    sig, seq, _, _ = parity_data["dna_r10_400bps"]
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    al.set_rescale(2)
    al.set_event_stats(True)
    a, xa = run_batch(al, sig, seq)
    b, xb = run_batch(al, sig, seq)
    same_results(a, b, levels=True, rescale=True)
    for u, v in zip(xa, xb):
        assert np.array_equal(_bits(u), _bits(v))
    # the same batch aligned again starts from x0 again, with the switch on or off
    with al.batch(sig, seq) as bt:
        bt.align(True)
        first = bt.fetch()
        al.set_rescale(0)
        bt.align(True)
        off = bt.fetch()
        x_off = bt.signals()
        al.set_rescale(2)
        bt.align(True)
        again = bt.fetch()
    same_results(first, again, levels=True, rescale=True)
    assert off.rescale_shift is None
    assert np.array_equal(_bits(x_off), _bits(np.concatenate(sig)))
    al.close()


def test_with_event_stats_the_levels_are_of_x_K(models, parity_data):
    sig, seq, _, _ = parity_data["rna004"]
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_rescale(2)
    al.set_event_stats(True)
    res, xs = run_batch(al, sig, seq)
    for i in range(res.n):
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i] + res.n_segments[i])
        want = levels_of(xs[i], res.signal_positions[a:b])
        got = np.stack([res.level_mean[a:b], res.level_stdv[a:b], res.level_median[a:b]])
        assert np.array_equal(_bits(got), _bits(want)), i
    al.close()


def test_recovery(models, parity_data):
    for pore in PORES:
        sig, seq, clean, _ = parity_data[pore]
        al = Aligner(models["syn9"], pore, device=0)
        ref = al.align_batch(clean[:48], seq[:48], True)
        for K in (0, RECOVERY_ITERS):
            al.set_rescale(K)
            res = al.align_batch(sig, seq, True)
            for j, (bb, aa) in enumerate(DISTORTIONS):
                idx = range(48 * (j + 1), 48 * (j + 2))
                agr = np.mean([border_agreement(res.read(i)["signal_positions"], ref.read(i % 48)["signal_positions"]) for i in idx])
                B = np.array([res.rescale_scale[i] if K else 1.0 for i in idx])
                A = np.array([res.rescale_shift[i] if K else 0.0 for i in idx])
                close = np.abs(B - bb).max() <= RECOVERY_PARAM_TOL and np.abs(A - aa).max() <= RECOVERY_PARAM_TOL
                if K:
                    assert close and agr >= RECOVERY_AGREEMENT, (pore, bb, aa, agr)
                else:
                    assert not close and agr < RECOVERY_AGREEMENT, (pore, bb, aa, agr)
        al.close()


def _fixed_dwell_read(rng, mean_c, sd_c, k, dwells, noise=0.05):
    n = len(dwells) + k - 1
    digits = rng.integers(0, 4, size=n)
    codes = synth._seq_codes(digits, k)
    idx = np.repeat(codes, dwells)
    x = mean_c[idx] + noise * sd_c[idx] * rng.standard_normal(len(idx))
    return np.ascontiguousarray(x), "".join(synth.BASES[d] for d in digits)


def test_guards(models):
    """< 16 rows, a constant signal and a permuted signal get no fit; a read with an invalid base keeps its message"""
    pore = "rna004"
    model = models["syn9"]
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(7400, 8, pore, mean, sd, (60, 150))
    sig = [r.signal for r in reads]
    seq = [r.sequence for r in reads]
    short = synth.make_reads(7401, 1, pore, mean, sd, 9 + 14)[0]        # 15 k-mers: 15 rows
    sig[0], seq[0] = short.signal, short.sequence
    sig[1] = np.full(len(sig[1]), 0.25)                                 # constant
    sig[2] = np.sort(sig[2])   # permuted into ascending order (a random shuffle still fits: the borders follow the model)
    seq[3] = seq[3][:30] + "N" + seq[3][31:]                            # invalid base
    chains = _chains(model, pore, sig, seq, 2)
    orc = Oracle(model, 1)
    r2 = chains[2][0]["res"]
    assert r2 is not None and not fit(row_model_means(r2, orc.table()[0], orc.kmers(seq[2]), 9),
                                      segment_means(sig[2], r2["signal_positions"]))[2]
    al = Aligner(model, pore, device=0)
    base = al.align_batch(sig, seq, True)
    al.set_rescale(2)
    res, xs = run_batch(al, sig, seq)
    check_chain(res, xs, chains, 2)
    assert res.status[3] != 0 and res.error(3) == base.error(3)
    for i in range(4):
        assert res.rescale_iters[i] == 0 and res.rescale_shift[i] == 0.0 and res.rescale_scale[i] == 1.0
        assert np.array_equal(_bits(xs[i]), _bits(sig[i]))
        if base.status[i] == 0:
            got, want = res.read(i), base.read(i)
            assert np.array_equal(got["signal_positions"], want["signal_positions"])
            assert np.array_equal(_bits(got["probabilities"]), _bits(want["probabilities"])) and got["Z"] == want["Z"]
    assert (res.rescale_iters[4:] >= 1).all()
    al.close()


def test_refusals(models):
    pore = "rna004"
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(7500, 5, pore, mean, sd, (60, 200))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn9"], pore, device=0)
    arrs = (np.zeros(16), np.zeros(16), np.zeros(16, dtype=np.int32))
    out = N.DynRescaleOut(arrs[0].ctypes.data_as(N.c_double_p), arrs[1].ctypes.data_as(N.c_double_p),
                          arrs[2].ctypes.data_as(N.c_i32_p), 16)
    with al.batch(sig, seq) as b:
        b.align(True)                         # switch off at submission
        al.set_rescale(1)
        with pytest.raises(ValueError, match="without dyn_aligner_set_rescale"):
            b.fetch_rescale(out)
        b.align(False)                        # Z only, switch on
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_rescale(out)
        assert b.fetch().rescale_shift is None
        b.align(True)
        b.fetch_rescale(out)
        assert (arrs[2][:5] >= 0).all() and (arrs[1][:5] > 0).all()
    t = al.align_async(*synth.pack_reads(reads), False)
    assert t.wait().rescale_shift is None
    with pytest.raises(ValueError, match="calc_probabilities"):
        t.fetch_rescale(out)
    t.close()
    al.close()


def test_async_merged_tickets_with_different_settings(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = []
    for j in range(8):
        reads = synth.make_reads(7600 + j, 300, "rna004", mean, sd, (150, 300))
        data.append((reads, synth.pack_reads(reads)))
    al = Aligner(models["syn9"], "rna004", device=0)
    want = {}
    for K in (1, 2):
        al.set_rescale(K)
        want[K] = [al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True) for reads, _ in data]
    merged = False
    for attempt in range(3):   # (whether tickets meet in the queue is a matter of timing)
        tickets = []
        for j, (_, packed) in enumerate(data):
            al.set_rescale(1 if j < 4 else 2)   # two settings in flight at once
            tickets.append(al.align_async(*packed, True))
        for j, t in enumerate(tickets):
            res = t.wait()
            same_results(res, want[1 if j < 4 else 2][j], rescale=True)
            merged |= t.timing()["launch_share"] < 1.0
            assert t.timing()["launches"] == 1
            t.close()
        if merged:
            break
    assert merged
    al.close()


def test_raw_async_device_preprocessing(models):
    pore = "rna004"
    model = models["syn9"]
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(7700, 24, pore, mean, sd, (80, 200))
    rng = np.random.default_rng(4)
    shift = rng.uniform(80, 100, len(reads))
    scale = rng.uniform(10, 20, len(reads))
    # the signal after the basecaller's shift / scale is off by an affine error of its own
    raw = [((1.15 * r.signal + 0.25) * sc + sh).astype(np.float32) for r, sh, sc in zip(reads, shift, scale)]
    seq = [r.sequence for r in reads]
    al = Aligner(model, pore, device=0)
    with al.batch_raw(raw, seq, shift, scale) as b:   # x0: the device-preprocessed signal of a K = 0 batch
        x = b.signals()
    sl = _slices([len(v) for v in raw])
    x0 = [x[s] for s in sl]
    chains = _chains(model, pore, x0, seq, 2)
    seqs = "".join(seq).encode()
    seq_off = np.zeros(len(seq) + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seq])
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in raw])
    al.set_rescale(2)
    t = al.align_raw_async(np.concatenate(raw), off, shift, scale, seqs, seq_off)
    res = t.wait()
    assert (res.status == 0).all()
    check_chain(res, None, chains, 2)
    assert (res.rescale_iters >= 1).all()
    t.close()
    al.close()


def test_wide_band_and_stall_segments(models):
    """band-600 reads on a wide handle (the generic kernel) beside ordinary ones, and reads with stalls of 300 .. 20 000
    samples (the fit's workgroup-wide segment means)"""
    pore = "rna004"
    model = models["syn9"]
    _, mean, sd = synth.read_model_file(model)
    mean_c, sd_c = synth.code_order_table(mean, sd, 9, True)
    rng = np.random.default_rng(8)
    wide = synth.make_reads(7800, 3, pore, mean, sd, (600, 700))
    normal = synth.make_reads(7801, 3, pore, mean, sd, (60, 200))
    sig = [1.1 * r.signal - 0.15 for r in wide + normal]
    seq = [r.sequence for r in wide + normal]
    for j, stall in enumerate((300, 2000, 20000)):
        dw = np.maximum(2, rng.poisson(10, size=120))
        dw[40] = stall
        dw[80] = 257 + j
        x, s = _fixed_dwell_read(rng, mean_c, sd_c, 9, dw)
        sig.append(0.9 * x + 0.1)
        seq.append(s)
    chains = _chains(model, pore, sig, seq, 2, band=1000)
    al = Aligner(model, pore, band=1000, device=0)
    al.set_rescale(2)
    res, xs = run_batch(al, sig, seq)
    assert (res.status == 0).all()
    check_chain(res, xs, chains, 2)
    assert (res.rescale_iters >= 1).all()
    L = np.concatenate([np.diff(np.append(res.read(i)["signal_positions"].astype(np.int64), len(sig[i]))) for i in range(6, 9)])
    assert (L > 256).sum() >= 3
    al.close()


def test_paged_launch(models, monkeypatch):
    monkeypatch.setenv("DYN_FORCE_LAYOUT", "separate")   # (a starved pool may pick the in-place posterior layout otherwise)
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(7900, 1200, "rna004", mean, sd, (100, 420))
    sig, seq = [0.95 * r.signal + 0.1 for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn9"], "rna004", device=0)
    al.set_rescale(1)
    with al.batch(sig, seq) as b:
        b.align(True)
        want = b.fetch()
        tw = b.timing()
    small = Aligner(models["syn9"], "rna004", device=0)
    small.set_mem_budget(2 << 30)
    small.set_rescale(1)
    with small.batch(sig, seq) as b:
        b.align(True)
        got = b.fetch()
        tg = b.timing()
    assert tg["pool_pages"] * tg["page_rows"] < tw["pool_pages"] * tw["page_rows"]   # the queue waited for pages
    same_results(got, want, rescale=True)
    assert (got.rescale_iters == 1).all()
    al.close()
    small.close()
